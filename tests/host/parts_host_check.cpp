// parts_host_check.cpp -- the host code of c3_predict_submit_parts / c3_predict_wait without a device: plan_batch, fill_parts, record_batch and
// scatter_parts (clair3_amd/csrc/c3_hostring.h) driven against plain host buffers that are exactly as large as the plan says, so that a
// byte read or written outside them is an error under AddressSanitizer.  Stand-alone, host only:
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -DC3HIP_SRC_HASH='"host-check"' tests/host/parts_host_check.cpp -o parts_host_check && ./parts_host_check
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

static void one_batch(c3_model *m, int x_dtype, const std::vector<int64_t> &counts, std::mt19937 &rng) {
    const size_t wbytes = (size_t)c3_model_window_bytes(m, x_dtype), row_bytes = (size_t)m->row * sizeof(float);
    const int n = (int)counts.size();
    std::vector<std::vector<uint8_t>> x(n);
    std::vector<std::vector<float>> y(n);
    std::vector<const void *> xp(n);
    std::vector<float *> yp(n);
    std::vector<uint8_t> all;
    int64_t batch = 0;
    for (int i = 0; i < n; ++i) {
        x[i].resize((size_t)counts[i] * wbytes);  // exactly the part: one byte further is an error
        for (uint8_t &b : x[i]) b = (uint8_t)rng();
        all.insert(all.end(), x[i].begin(), x[i].end());
        y[i].assign((size_t)counts[i] * m->row, -1.f);
        xp[i] = counts[i] ? x[i].data() : nullptr, yp[i] = counts[i] ? y[i].data() : nullptr;  // (an empty part's pointers are not read)
        batch += counts[i];
    }
    RingInput in = ring_input(InKind::Parts, nullptr, x_dtype, batch, nullptr);
    in.parts = xp.data(), in.counts = counts.data(), in.y_parts = yp.data(), in.n_parts = n;
    const StagedBatch p = plan_batch(m, in, false);
    CHECK(p.image.off == 0 && p.image.bytes == all.size() && p.staged == all.size() && p.x_cap == all.size());
    CHECK(p.y.off == 0 && p.y.bytes == (size_t)batch * row_bytes && p.y_total == p.y.bytes);
    CHECK(p.depth.bytes == 0 && p.starts.bytes == 0 && p.rows_tab.bytes == 0 && p.cand_pos.bytes == 0);
    HostSlot sl;
    std::vector<uint8_t> pin_x(p.x_cap);
    std::vector<float> pin_y(p.y_total / sizeof(float));
    sl.pin_x = pin_x.data(), sl.pin_y = pin_y.data();
    Filled f;
    fill_parts(sl, in, p, wbytes, f);
    CHECK(f.src == nullptr && f.nrun == 1 && f.run[0].off == 0 && f.run[0].bytes == p.image.bytes);
    CHECK(pin_x == all);
    record_batch(m, sl, in, p, -1);
    CHECK(sl.busy && sl.batch == batch && sl.n_parts == n);
    // the caller's tables may be reused as soon as submit returns: the slot has its own copy
    std::vector<float *> yp_kept = yp;
    std::fill(xp.begin(), xp.end(), nullptr), std::fill(yp.begin(), yp.end(), nullptr);
    for (size_t i = 0; i < pin_y.size(); ++i) pin_y[i] = (float)i;
    scatter_parts(sl, row_bytes);
    size_t at = 0;
    for (int i = 0; i < n; ++i)
        for (size_t k = 0; k < y[i].size(); ++k, ++at) CHECK(y[i][k] == (float)at);
    CHECK(at == pin_y.size());
    // a batch from ONE buffer that follows in the same slot is no batch of parts
    RingInput plain = ring_input(InKind::Sliced, all.data(), x_dtype, batch, pin_y.data());
    record_batch(m, sl, plain, plan_batch(m, plain, false), -1);
    CHECK(sl.n_parts == 0);
    (void)yp_kept;
}

int main() {
    std::mt19937 rng(7);
    c3_model *pileup = new c3_model(), *fa = new c3_model();
    pileup->kind = C3_KIND_PILEUP, pileup->C = 18, pileup->nout = 24, pileup->row = 24;
    fa->kind = C3_KIND_FULL_ALIGNMENT, fa->C = 9, fa->depth = 55, fa->nout = 90, fa->row = 90 + kDecodeCols;  // (odd window and row sizes)
    for (int dt : {C3_DTYPE_I8, C3_DTYPE_I32}) {
        one_batch(pileup, dt, {1, 7, 16, 17, 0}, rng);
        one_batch(pileup, dt, {0}, rng);
        one_batch(pileup, dt, {0, 0, 5, 0}, rng);
        one_batch(pileup, dt, std::vector<int64_t>(kMaxParts, 3), rng);
        one_batch(pileup, dt, {4000, 1, 2500}, rng);  // parts beyond 512 KiB: the staging pool's helpers copy them in pieces
    }
    one_batch(fa, C3_DTYPE_I8, {1, 2, 3, 0}, rng);
    one_batch(fa, C3_DTYPE_I8, {130, 0, 1, 77}, rng);  // 2.1 MB and 1.3 MB parts
    for (int k = 0; k < 20; ++k) {
        std::vector<int64_t> counts(1 + rng() % kMaxParts);
        for (int64_t &c : counts) c = rng() % 4 == 0 ? 0 : rng() % 40;
        one_batch(k % 2 ? fa : pileup, C3_DTYPE_I8, counts, rng);
    }
    delete pileup;
    delete fa;
    printf("parts_host_check: %d failure(s)\n", failures);
    return failures != 0;
}
