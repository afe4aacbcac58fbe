// c3_rescale.h -- the reference's rule for pileup windows of very deep coverage, on the device.  Both in-process loops of the
// reference bring a window down to max_depth before the network sees it (clair3/CallVariantsFromCffi.py:278-285, clair3/utils.py:104-111;
// max_depth = shared/param_p.py:15 = 144):
//     depth = int(alt_info.split('-', 1)[0])
//     if depth > 0 and depth > max_depth * 1.5:  X[i] = X[i] / (depth / max_depth)      # int32 array: truncated towards zero
// i.e. TWO roundings in double -- s = depth / max_depth, then x / s -- and not the exact rational trunc(x * max_depth / depth): the two
// differ for x = 217, depth = 248 (125 against 126).  The library is compiled without fast-math (clair3_amd/build.py FLAGS), so both
// divisions below are IEEE correctly rounded and the double -> int32 conversion truncates, like numpy's cast; do not replace them by
// a reciprocal multiply.
//
// A pre-pass, not a flag of lstm1_fused_kernel: that kernel is persistent and latency-bound with ~150 resident weight registers
// (c3_lstm_fused.h), 594 double divisions per window do not belong in its time-step loop.  The pre-pass writes the SLICED windows of a
// micro-batch -- gathered out of the region matrix where the batch has `starts` -- into the lane's workspace and the int32 form of
// lstm1_fused_kernel runs on that buffer unchanged.  The staged input of the slot is never written: the range guard's re-run
// (c3_hostring.h c3_predict_wait) rescales again from the original counts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

struct RescaleParams {
    const int32_t *x;       // sliced windows [B][T][C], or with `starts` the region matrix [n_cols][C]
    const int32_t *starts;  // first column of window b in the region matrix (nullptr: sliced windows)
    const int32_t *depth;   // [B]
    int32_t *out;           // [B][T][C]
    int B, TC, C;           // windows, counts per window (T * C), counts per column
    int max_depth;
};

constexpr int kRescaleThreads = 256;
constexpr int kRescaleWindows = 4;  // windows per workgroup: one wave each (a window of 33 x 18 counts = 297 int2: five passes of 64 lanes)

// One wave per window: the rescale decision is wave-uniform (no divergence, windows that are not rescaled never reach the divisions).
// V = 2: int2 loads and stores.  A window starts at a multiple of C counts in either input (72 bytes for C = 18) and its rows are
// contiguous in the region matrix too, so with C even every window is one 8-byte aligned run of T * C counts: consecutive lanes read
// consecutive int2 -- whole 64-byte segments apart from the run's ends.  V = 1 for an odd channel count.
template <int V>
__global__ __launch_bounds__(kRescaleThreads) void rescale_windows_kernel(RescaleParams p) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * kRescaleWindows + (threadIdx.x >> 6);
    if (b >= p.B) return;
    const int32_t d = p.depth[b];
    const int32_t *src = p.x + (p.starts ? (int64_t)p.starts[b] * p.C : (int64_t)b * p.TC);
    int32_t *dst = p.out + (int64_t)b * p.TC;
    // depth > 1.5 * max_depth, as the reference compares it (int against float; exact in double for every int32)
    const bool deep = d > 0 && (double)d > 1.5 * (double)p.max_depth;
    const double s = (double)d / (double)p.max_depth;  // first rounding: Python's int / int
    if constexpr (V == 2) {
        const int2 *s2 = reinterpret_cast<const int2 *>(src);
        int2 *d2 = reinterpret_cast<int2 *>(dst);
        for (int i = lane; i < p.TC / 2; i += 64) {
            int2 v = s2[i];
            if (deep) v.x = (int32_t)((double)v.x / s), v.y = (int32_t)((double)v.y / s);  // second rounding, then towards zero
            d2[i] = v;
        }
    } else {
        for (int i = lane; i < p.TC; i += 64) {
            int32_t v = src[i];
            if (deep) v = (int32_t)((double)v / s);
            dst[i] = v;
        }
    }
}

}  // namespace c3
