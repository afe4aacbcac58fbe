// score_host_check.cpp -- the host code of c3_score_submit / c3_score_wait without a device: plan_batch for a scored batch, the fills
// (fill_sliced, fill_labels), record_batch and the record reader (read_score) of clair3_amd/csrc/c3_hostring.h, driven against plain host
// buffers that are exactly as large as the plan says, so that a byte read or written outside them is an error under AddressSanitizer.
// Stand-alone, host only:
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -DC3HIP_SRC_HASH='"host-check"' tests/host/score_host_check.cpp -o score_host_check && ./score_host_check
//
// (the library's one translation unit, so the device code is compiled along; it is not run.)  No HIP call is made and no device is needed:
// the slot's "pinned" buffers are malloc'ed here.
#include "../../clair3_amd/csrc/c3_model.hip"

#include <cstdio>
#include <random>

using namespace c3;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) ++failures, fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    } while (0)

static void one_batch(c3_model *m, int x_dtype, int64_t batch, int label_dtype, bool want_rows, bool want_losses, bool with_depth, bool verify,
                      std::mt19937 &rng) {
    want_rows &= batch > 0, want_losses &= batch > 0;  // (the buffers of an empty batch are null pointers)
    const size_t wbytes = (size_t)c3_model_window_bytes(m, x_dtype), lsize = label_dtype == C3_DTYPE_F32 ? 4 : 1;
    std::vector<uint8_t> x((size_t)batch * wbytes), labels((size_t)batch * m->nout * lsize);  // exactly the batch: one byte further is an error
    for (uint8_t &b : x) b = (uint8_t)rng();
    for (uint8_t &b : labels) b = (uint8_t)rng();
    std::vector<int32_t> depth((size_t)batch, 7);
    std::vector<float> y((size_t)batch * m->row, -1.f), losses((size_t)batch * m->nb, -1.f);
    RingInput in = ring_input(InKind::Sliced, x.data(), x_dtype, batch, want_rows ? y.data() : nullptr, with_depth ? depth.data() : nullptr);
    in.score = true, in.labels = labels.data(), in.label_dtype = label_dtype, in.loss_host = want_losses ? losses.data() : nullptr;
    const StagedBatch p = plan_batch(m, in, with_depth, verify, false);
    // the layout: every section from a multiple of 256 bytes, in order, nothing overlapping, the labels the last thing staged
    CHECK(p.image.off == 0 && p.image.bytes == x.size());
    CHECK(p.labels.bytes == labels.size() && p.labels.off % 256 == 0 && p.labels.off >= p.image.bytes);
    if (with_depth) CHECK(p.depth.bytes == (size_t)batch * 4 && p.depth.off % 256 == 0 && p.depth.off >= p.image.bytes && p.depth.off + p.depth.bytes <= p.labels.off);
    CHECK(p.staged == p.labels.off + p.labels.bytes && p.x_cap == p.staged && p.tail <= p.labels.off && p.tail >= p.image.bytes);
    CHECK(p.y.off == 0 && p.y.bytes == (size_t)batch * m->row * sizeof(float));
    if (verify) CHECK(p.verify.bytes == kVerifyRecordBytes && p.verify.off % 256 == 0 && p.verify.off >= p.y.bytes && p.verify.off + p.verify.bytes <= p.score.off);
    CHECK(p.score.bytes == kScoreRecordBytes && p.score.off % 256 == 0 && p.score.off >= p.y.bytes && sizeof(ScoreRecord) <= kScoreRecordBytes);
    CHECK(p.losses.bytes == (want_losses ? (size_t)batch * m->nb * sizeof(float) : 0));
    if (want_losses) CHECK(p.losses.off == p.score.off + p.score.bytes && p.losses.off % 256 == 0);
    CHECK(p.y_total == (want_losses ? p.losses.off + p.losses.bytes : p.score.off + p.score.bytes));
    // an unscored batch of the same input is laid out as before
    RingInput plain = in;
    plain.score = false, plain.labels = nullptr, plain.loss_host = nullptr, plain.y_host = y.data();
    const StagedBatch q = plan_batch(m, plain, with_depth, verify, false);
    CHECK(q.labels.bytes == 0 && q.score.bytes == 0 && q.losses.bytes == 0);
    CHECK(q.staged == (with_depth ? q.depth.off + q.depth.bytes : q.image.bytes) && q.y_total == (verify ? q.verify.off + q.verify.bytes : q.y.bytes));

    HostSlot sl;
    std::vector<uint8_t> pin_x(p.x_cap), pin_y(p.y_total);
    sl.pin_x = pin_x.data(), sl.pin_y = (float *)pin_y.data();
    Filled f;
    fill_sliced(sl, in, p, with_depth ? depth.data() : nullptr, f);
    fill_labels(sl, in, p);
    CHECK(f.src == x.data() && f.nrun == 0);
    CHECK(batch == 0 || memcmp(pin_x.data() + p.labels.off, labels.data(), labels.size()) == 0);
    if (with_depth && batch) CHECK(memcmp(pin_x.data() + p.depth.off, depth.data(), p.depth.bytes) == 0);
    record_batch(m, sl, in, p, -1);
    CHECK(sl.busy && sl.scored && sl.rows_home == !want_rows && sl.label_dtype == label_dtype && sl.score_rec.windows == 0 && sl.score_rec.tasks == m->nb);
    // the reader: the record the device would have written, and the windows' values
    ScoreRecord rec = ScoreRecord{};
    rec.windows = (int32_t)batch, rec.tasks = m->nb, rec.nonfinite = 3;
    for (int k = 0; k < 4; ++k) rec.loss_sum[k] = 1.5 * (k + 1), rec.correct[k] = 10 + k;
    memcpy(pin_y.data() + p.score.off, &rec, sizeof(rec));
    for (size_t i = 0; want_losses && i < (size_t)batch * m->nb; ++i) {
        const float v = (float)i;
        memcpy(pin_y.data() + p.losses.off + 4 * i, &v, 4);
    }
    read_score(sl);
    CHECK(memcmp(&sl.score_rec, &rec, sizeof(rec)) == 0);
    for (size_t i = 0; i < losses.size(); ++i) CHECK(losses[i] == (want_losses ? (float)i : -1.f));
    c3_score_result out;
    score_result(m, sl.score_rec, &out);
    CHECK(out.windows == batch && out.tasks == m->nb && out.nonfinite == 3 && out.loss_sum[3] == 6.0 && out.correct[0] == 10);
    // a batch that is not scored and follows in the same slot is no scored batch
    record_batch(m, sl, plain, q, -1);
    CHECK(!sl.scored && !sl.rows_home && sl.loss_host == nullptr);
}

int main() {
    std::mt19937 rng(11);
    c3_model *pileup = new c3_model(), *pileup4 = new c3_model(), *fa = new c3_model();
    pileup->kind = C3_KIND_PILEUP, pileup->C = 18, pileup->nb = 2, pileup->nout = 24, pileup->row = 24;
    pileup4->kind = C3_KIND_PILEUP, pileup4->C = 18, pileup4->nb = 4, pileup4->nout = 90, pileup4->row = 90;
    fa->kind = C3_KIND_FULL_ALIGNMENT, fa->C = 9, fa->depth = 55, fa->nb = 4, fa->nout = 90, fa->row = 90 + kDecodeCols;  // (odd window and row sizes)
    for (int64_t batch : {0, 1, 3, 65, 257, 1000})
        for (int ld : {C3_DTYPE_I8, C3_DTYPE_F32})
            for (int mask = 0; mask < 8; ++mask) {
                one_batch(pileup, C3_DTYPE_I8, batch, ld, mask & 1, mask & 2, false, mask & 4, rng);
                one_batch(pileup4, C3_DTYPE_I32, batch, ld, mask & 1, mask & 2, (mask & 4) && batch > 0, false, rng);
                if (batch <= 65) one_batch(fa, C3_DTYPE_I8, batch, ld, mask & 1, mask & 2, false, mask & 4, rng);
            }
    delete pileup;
    delete pileup4;
    delete fa;
    printf("score_host_check: %d failure(s)\n", failures);
    return failures != 0;
}
