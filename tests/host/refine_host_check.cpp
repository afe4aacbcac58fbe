// refine_host_check.cpp -- the host code of refine mode (clair3_amd/csrc/c3_refine.h) without a device: plan_batch with and without the refine
// section (every other section stays what it was), which batches the mode covers, record_batch and c3_predict_wait's accounting of a batch
// that came home (refine_account: skipped batches, a record with nothing selected, a record that cannot be right), the scratch layout of the
// selection, and the entries' refusals -- driven against plain host buffers that are exactly as large as the plan says, so that a byte read
// or written outside them is an error under AddressSanitizer.  Stand-alone, host only:
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -DC3HIP_SRC_HASH='"host-check"' tests/host/refine_host_check.cpp -o refine_host_check && ./refine_host_check
//
// (the library's one translation unit, so the device code is compiled along; it is not run.)  No HIP call is made and no device is needed:
// the slot's "pinned" buffers are malloc'ed here, and no record of these batches selects a window (the second pass is the device's).
#include "../../clair3_amd/csrc/c3_model.hip"

#include <cstdio>

using namespace c3;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) ++failures, fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    } while (0)

static void one_batch(c3_model *m, int64_t batch, bool on_device, bool parts) {
    const size_t wbytes = (size_t)c3_model_window_bytes(m, C3_DTYPE_I8);
    std::vector<uint8_t> x((size_t)batch * wbytes);
    std::vector<float> y((size_t)batch * m->row, -1.f);
    float dev_rows = 0.f;  // (stands for the caller's device buffer: never dereferenced)
    RingInput in = ring_input(parts ? InKind::Parts : InKind::Sliced, x.data(), C3_DTYPE_I8, batch, on_device ? nullptr : y.data(), nullptr, on_device ? &dev_rows : nullptr);
    m->refine_on = false;
    CHECK(!refine_covers(m, in));
    const StagedBatch off = plan_batch(m, in, false, false, false, refine_covers(m, in));
    CHECK(off.refine.bytes == 0 && off.refine.off == 0 && off.y_total == off.y.bytes);
    m->refine_on = true;
    CHECK(refine_covers(m, in) == (batch > 0));
    const StagedBatch p = plan_batch(m, in, false, false, false, refine_covers(m, in));
    CHECK(p.image.bytes == off.image.bytes && p.staged == off.staged && p.x_cap == off.x_cap && p.y.bytes == off.y.bytes && p.y.off == 0);
    if (batch == 0) {
        CHECK(p.refine.bytes == 0 && p.y_total == off.y_total);
        return;
    }
    CHECK(p.refine.bytes == kRefineRecordBytes + (((size_t)batch * 4 + 15) & ~(size_t)15) && p.refine.bytes % 16 == 0);
    if (on_device) CHECK(p.refine.off == 0 && p.y_total == p.refine.bytes);  // all the slot's output buffer holds
    else CHECK(p.refine.off % 256 == 0 && p.refine.off >= off.y_total && p.refine.off < off.y_total + 256 && p.y_total == p.refine.off + p.refine.bytes);
    // the scratch of the selection: three arrays that do not overlap, inside the allocation
    const RefineScratch at(batch);
    CHECK(at.gaps_at == 0 && at.bits_at >= (size_t)batch * 4 && at.part_at >= at.bits_at + (size_t)batch && at.part_at % 256 == 0);
    CHECK(at.bytes == at.part_at + (size_t)refine_blocks(batch) * sizeof(RefinePart) && (int64_t)refine_blocks(batch) * kRefineWindows >= batch);

    // the accounting of a batch that came home, against buffers of exactly the plan's size
    HostSlot sl;
    std::vector<uint8_t> pin_y(on_device ? p.refine.bytes : p.y_total);
    sl.pin_y = (float *)pin_y.data();
    int64_t part_counts[1] = {batch};
    const void *part_x[1] = {x.data()};
    float *part_y[1] = {y.data()};
    if (parts) in.parts = part_x, in.counts = part_counts, in.y_parts = part_y, in.n_parts = 1;
    record_batch(m, sl, in, p, -1);
    CHECK(sl.refine_on && sl.plan.refine.bytes == p.refine.bytes);
    RefineRecord rec = RefineRecord{};
    rec.windows = (uint32_t)batch, rec.head[1] = 0, rec.min_gap[0] = 0.25f, rec.min_gap[1] = 0.5f, rec.min_gap[2] = rec.min_gap[3] = INFINITY;
    memcpy(pin_y.data() + p.refine.off, &rec, sizeof(rec));
    refine_zero(m);
    CHECK(refine_account(m, sl, false) == 0);
    const c3_refine_stats &t = m->rfstats;
    CHECK(t.batches == 1 && t.batches_refined == 0 && t.batches_skipped == 0 && t.windows == batch && t.windows_selected == 0);
    CHECK(t.min_gap[0] == 0.25f && t.min_gap[1] == 0.5f && std::isinf(t.min_gap[2]) && t.max_abs_diff == 0.f);
    CHECK(refine_account(m, sl, true) == 0 && t.batches == 2 && t.batches_skipped == 1 && t.windows == batch);  // the range guard answered it
    rec.windows = (uint32_t)batch + 1;  // a record that cannot be this batch's
    memcpy(pin_y.data() + p.refine.off, &rec, sizeof(rec));
    CHECK(refine_account(m, sl, false) != 0 && strstr(c3_last_error(), "internal") && t.windows == batch);
    rec.windows = (uint32_t)batch, rec.selected = (uint32_t)batch + 1;
    memcpy(pin_y.data() + p.refine.off, &rec, sizeof(rec));
    CHECK(refine_account(m, sl, false) != 0 && strstr(c3_last_error(), "internal"));
    // a batch planned while the mode was off: counted as skipped when it comes home with the mode on, nothing read behind its buffer
    std::vector<uint8_t> small_y(std::max<size_t>(off.y_total, 1));
    sl.pin_y = (float *)small_y.data();
    record_batch(m, sl, in, off, -1);
    refine_zero(m);
    CHECK(refine_account(m, sl, false) == 0 && t.batches == 1 && t.batches_skipped == 1 && t.windows == 0);
}

static void coverage(c3_model *m) {
    uint8_t x[4] = {};
    float y[4] = {};
    int32_t depth[1] = {7};
    m->refine_on = true, m->answer_exact = false;
    RingInput in = ring_input(InKind::Sliced, x, C3_DTYPE_I8, 1, y);
    CHECK(refine_covers(m, in));
    for (InKind k : {InKind::Region, InKind::Candidates, InKind::Rows, InKind::PackedHere}) {
        RingInput other = in;
        other.kind = k;
        CHECK(!refine_covers(m, other));
    }
    RingInput deep = in, scored = in, big = in;
    deep.depth = depth, scored.score = true, big.batch = kRefineMaxBatch + 1;
    CHECK(!refine_covers(m, deep) && !refine_covers(m, scored) && !refine_covers(m, big));
    big.batch = kRefineMaxBatch;
    CHECK(refine_covers(m, big));
    m->answer_exact = true;
    CHECK(!refine_covers(m, in));
    m->answer_exact = false;
}

static void entries(c3_model *m) {
    c3_refine_stats out;
    int64_t n = -1;
    m->refine_on = m->refine_seen = false, m->exact.loaded = false, m->verify_every = 0;
    CHECK(c3_model_set_refine(nullptr, 1, 1e-4f) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_model_refine_stats(nullptr, &out) != 0 && c3_model_refine_stats(m, nullptr) != 0 && c3_model_refine_reset(nullptr) != 0);
    CHECK(c3_model_set_refine(m, 1, -1.f) != 0 && strstr(c3_last_error(), "gap must be"));
    CHECK(c3_model_set_refine(m, 1, NAN) != 0 && c3_model_set_refine(m, 1, INFINITY) != 0 && !m->refine_on);
    CHECK(c3_model_set_refine(m, 1, 1e-4f) != 0 && strstr(c3_last_error(), "the exact form was not enabled at the last load"));
    m->exact.loaded = true, m->exact.want = true;
    m->verify_every = 4;
    CHECK(c3_model_set_refine(m, 1, 1e-4f) != 0 && strstr(c3_last_error(), "verify mode is on") && !m->refine_on);
    m->verify_every = 0;
    m->slot[1].busy = true;
    CHECK(c3_model_set_refine(m, 1, 1e-4f) != 0 && strstr(c3_last_error(), "in flight") && c3_model_refine_reset(m) != 0);
    m->slot[1].busy = false;
    CHECK(c3_model_refine_stats(m, &out) == 0 && out.batches == 0 && out.gap == 0.f && std::isinf(out.min_gap[3]));
    CHECK(c3_model_set_refine(m, 1, 0.f) == 0 && m->refine_on && m->refine_gap == 0.f);
    CHECK(c3_model_set_refine(m, 1, 1e-4f) == 0 && m->refine_on && m->refine_seen && m->refine_gap == 1e-4f);
    CHECK(c3_model_set_verify(m, 2, 1e-4f, 1e-6f, C3_VERIFY_REPORT) != 0 && strstr(c3_last_error(), "refine mode is on") && m->verify_every == 0);
    CHECK(c3_model_set_verify(m, 0, 1e-4f, 1e-6f, C3_VERIFY_REPORT) == 0);  // (switching verify mode off is no conflict)
    CHECK(c3_model_set_exact(m, 0) != 0 && strstr(c3_last_error(), "refine mode") && m->exact.want);
    m->rfstats.batches = 3, m->rfstats.windows_selected = 2, m->rfstats.min_gap[1] = 0.125f;
    CHECK(c3_model_set_refine(m, 0, 0.f) == 0 && !m->refine_on);  // off: the totals stay readable
    CHECK(c3_model_refine_stats(m, &out) == 0 && out.batches == 3 && out.windows_selected == 2 && out.min_gap[1] == 0.125f && out.gap == 1e-4f);
    char text[1024];
    CHECK(c3_model_describe(m, text, sizeof(text)) == 0 && !strstr(text, "refine="));
    CHECK(c3_model_set_refine(m, 1, 0.5f) == 0 && m->rfstats.batches == 3);  // on again: they go on
    CHECK(c3_model_describe(m, text, sizeof(text)) == 0 && strstr(text, " refine=gap:0.5,windows:0,selected:2,changed:0"));
    CHECK(c3_model_refine_reset(m) == 0 && c3_model_refine_stats(m, &out) == 0 && out.batches == 0 && std::isinf(out.min_gap[1]));
    CHECK(sizeof(c3_refine_stats) == 112 && sizeof(RefineRecord) == 256 && sizeof(RefinePart) == 40);
    // the selection alone: what it refuses before it touches the device
    int32_t index[2];
    float rows[4] = {};
    CHECK(c3_refine_select(nullptr, rows, 24, 1, 1e-4f, index, &n, nullptr) != 0 && c3_refine_select(m, rows, m->nout, 1, 1e-4f, index, nullptr, nullptr) != 0);
    CHECK(c3_refine_select(m, rows, m->nout + 1, 1, 1e-4f, index, &n, nullptr) != 0 && strstr(c3_last_error(), "rows of"));
    CHECK(c3_refine_select(m, rows, m->nout, -1, 1e-4f, index, &n, nullptr) != 0 && c3_refine_select(m, rows, m->nout, 1, -1.f, index, &n, nullptr) != 0);
    CHECK(c3_refine_select(m, rows, m->nout, kRefineMaxBatch + 1, 1e-4f, index, &n, nullptr) != 0 && strstr(c3_last_error(), "too many windows"));
    CHECK(c3_refine_select(m, nullptr, m->nout, 0, 1e-4f, nullptr, &n, nullptr) == 0 && n == 0);
    m->refine_on = false, m->exact.loaded = false, m->exact.want = false;
}

int main() {
    c3_model *pileup = new c3_model(), *fa = new c3_model();
    pileup->kind = C3_KIND_PILEUP, pileup->C = 18, pileup->nb = 2, pileup->nout = 24, pileup->row = 24;
    fa->kind = C3_KIND_FULL_ALIGNMENT, fa->C = 9, fa->depth = 55, fa->nb = 4, fa->nout = 90, fa->row = 90 + kDecodeCols;  // (odd window and row sizes)
    for (c3_model *m : {pileup, fa}) {
        entries(m);
        coverage(m);
        for (int64_t batch : {0, 1, 3, 63, 64, 65, 257, 1025})
            for (int mask = 0; mask < 4; ++mask) one_batch(m, batch, mask & 1, mask & 2);
        m->refine_on = false;
    }
    delete pileup;
    delete fa;
    printf("refine_host_check: %d failure(s)\n", failures);
    return failures != 0;
}
