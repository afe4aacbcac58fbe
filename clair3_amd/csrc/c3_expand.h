// c3_expand.h -- the zero rows of a full-alignment window, on the device.  A window is depth x 33 x C int8, but only the reads that
// overlap the candidate fill rows; the reference's stream format carries just those rows and its generator pads them to the matrix depth
// on the host before the model call (clair3/utils.py:113-121):
//     padding_depth = depth - tensor_depth;  prefix = int(padding_depth / 2);  suffix = padding_depth - prefix
// and its C producer lays the dense matrix out by the same rule (src/clair3_full_alignment_dwell.c:139-150, prefix_padding_depth =
// padding_depth >> 1).  The rows entries (c3_predict_submit_rows, c3_hostring.h) stage the occupied rows alone plus one table entry per
// window; this pre-pass writes the dense windows of a micro-batch into the lane's workspace and the unchanged forward pass -- both
// run_fa_planes and run_fa_fp32 read int8 windows through one pointer -- runs on that buffer.
//
// A pre-pass, not a source form of conv3x3_planes_kernel<..., SRC8>: res1a / res1b already carry 3.6 - 3.8 vector instructions per
// matrix instruction, a per-row indirection does not belong in their halo loaders.  The staged rows and the table are never
// written: the range guard's re-run (c3_hostring.h c3_predict_wait) expands again from them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

// one per window, filled by the host in its one pass over row_count
struct ExpandEntry {
    int64_t src;    // byte offset of the window's first occupied row in the staged rows
    int32_t first;  // dense row the run starts at
    int32_t count;  // rows of the run (0: an all-zero window)
};

struct ExpandParams {
    const int8_t *rows;      // the staged rows
    const ExpandEntry *tab;  // [B]
    int8_t *out;             // [B][depth][positions * C] dense windows
    int B;
    int row_bytes, window_bytes;  // positions * C, depth * row_bytes
};

constexpr int kExpandThreads = 256;

// One workgroup per window: the table entry is workgroup-uniform (scalar loads), and because the occupied rows are ONE run, destination
// piece p of the window is source piece p - lo for lo <= p < hi and zero elsewhere -- no division, no per-row lookup.  Every destination
// byte is written exactly once, zero or a source byte: no memset launch, no atomics.
// V = 8: 8-byte pieces.  With an even C, row bytes (264) and window bytes (23 496) are multiples of 8 and every buffer starts 256-aligned,
// so source and destination pieces are 8-byte aligned (window bytes are NOT a multiple of 16: every other window starts 8 off, so a
// 16-byte form would need a peeled first piece per window for 2 937 pieces of work).  V = 1: bytes, for an odd channel count (dwell: 297-
// byte rows, 26 433-byte windows), chosen the way rescale_windows_kernel<2> / <1> are.
template <int V>
__global__ __launch_bounds__(kExpandThreads) void expand_rows_kernel(ExpandParams p) {
    const int b = blockIdx.x;
    if (b >= p.B) return;
    const ExpandEntry e = p.tab[b];
    const int n = p.window_bytes / V;
    const int lo = e.first * (p.row_bytes / V), hi = lo + e.count * (p.row_bytes / V);
    if constexpr (V == 8) {
        const uint2 *src = reinterpret_cast<const uint2 *>(p.rows + e.src);
        uint2 *dst = reinterpret_cast<uint2 *>(p.out + (int64_t)b * p.window_bytes);
        for (int i = threadIdx.x; i < n; i += kExpandThreads) {
            uint2 v = make_uint2(0u, 0u);
            if (i >= lo && i < hi) v = src[i - lo];
            dst[i] = v;
        }
    } else {
        const int8_t *src = p.rows + e.src;
        int8_t *dst = p.out + (int64_t)b * p.window_bytes;
        for (int i = threadIdx.x; i < n; i += kExpandThreads) {
            int8_t v = 0;
            if (i >= lo && i < hi) v = src[i - lo];
            dst[i] = v;
        }
    }
}

}  // namespace c3
