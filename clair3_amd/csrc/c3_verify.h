// c3_verify.h -- verify mode (c3_model_set_verify): the rows of a batch as the fp16x3 forms computed them against the rows
// of the same staged input on the fp32-MFMA forms, compared where they are.
//
// Per row and head (columns (0,21) (21,24) (24,57) (57,90), limited to nout; the decoder columns behind nout are not compared), with the
// fp32 rows b as the reference -- the rule of tests/util.py label_mismatches:
//   |a - b| in fp32;  arg-max of a != arg-max of b (first maximum, as numpy's);  the top-2 gap of b in that head (largest minus second
//   largest value, 0 when the maximum occurs twice) <= near_tie: a differing arg-max is then excused as a near-tie.
// Over the batch: max |d| overall and per head, the lowest row that reaches the overall maximum, the rows with any |d| > tol, per head
// the arg-max differences outside near-ties and the excused ones.
//
// Two launches on the batch's stream behind the second forward pass:
//   rows_compare_kernel    four lanes per row, one per head; a row's maximum over its quad by two shuffles; every thread walks its rows in
//                          ascending order; then a butterfly over the 16 quads of a wave (per head: the xor distances are multiples of 4),
//                          the four waves through LDS, one partial per workgroup
//   rows_compare_final_kernel   one wave adds the workgroups' partials up and writes the batch's record into the slot's output buffer, from
//                          where it leaves with the rows (host_copy_kernel)
// No atomics; every combination is a maximum, an integer sum or the lexicographic (larger |d|, lower row): the record does not depend on
// scheduling or on the grid.
// Behind them (further down): the layer records of c3_model_set_verify_layers -- the same comparison per LAYER, layer_compare_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

constexpr int kVerifyThreads = 256;     // 64 rows per workgroup and pass
constexpr int kVerifyMaxBlocks = 1024;  // partials of one batch (a larger batch: every workgroup takes several passes)
constexpr size_t kVerifyRecordBytes = 256;  // the record's section of a staged batch (a multiple of 256 like every section)
// ... behind the record in that section (c3_exact.h writes them, c3_predict_wait reads them): the double maximum of a comparison with
// the exact rows, and the count of rows C3_VERIFY_REPLACE overwrote
constexpr size_t kVerifyMax64At = 64, kVerifyReplacedAt = 72;

struct VerifyRecord {  // 16 words: a workgroup's partial, and the batch's record as c3_predict_wait reads it
    float max_abs;
    float head_max[4];
    uint32_t worst_row;  // lowest row with max |d| == max_abs (0xffffffff: no row yet)
    uint32_t rows_over;
    uint32_t label[4];
    uint32_t tie[4];
    uint32_t n;  // rows compared (the final record only)
};

struct CompareParams {
    const float *a;        // the rows under test [batch][stride]
    const float *b;        // the fp32 forms' rows, same layout
    const uint32_t *kept;  // a candidate batch: the device word with the kept count -- only rows [0, kept) are compared; else nullptr
    VerifyRecord *part;    // [gridDim.x]
    int stride, nout, batch;
    float tol, near_tie;
};

__device__ __forceinline__ void verify_max_row(float &m, uint32_t &row, float om, uint32_t orow) {
    if (om > m || (om == m && orow < row)) m = om, row = orow;
}

// Both kernels go into a section of their own, which the linker puts behind `.text`: every other kernel keeps the address
// it had before these two existed (a shift of all of `.text` has cost the headline before: DESIGN.md 3.4)
#define C3_VERIFY_TEXT __attribute__((section(".c3_verify_text")))

__global__ __launch_bounds__(kVerifyThreads) C3_VERIFY_TEXT void rows_compare_kernel(CompareParams p) {
    __shared__ VerifyRecord wave_rec[kVerifyThreads / 64];
    const int tid = threadIdx.x, h = tid & 3, lane = tid & 63;
    const int lo = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
    const int hi = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
    const int n = p.kept ? (int)min(*p.kept, (uint32_t)p.batch) : p.batch;
    float t_max = 0.f, t_head = 0.f;
    uint32_t t_row = 0xffffffffu, t_over = 0, t_label = 0, t_tie = 0;
    for (int r0 = blockIdx.x * (kVerifyThreads / 4); r0 < n; r0 += gridDim.x * (kVerifyThreads / 4)) {  // (uniform over the workgroup)
        const int r = r0 + (tid >> 2);
        float d = 0.f;
        if (r < n && lo < hi) {
            const float *a = p.a + (int64_t)r * p.stride, *b = p.b + (int64_t)r * p.stride;
            float am = -INFINITY, b1 = -INFINITY, b2 = -INFINITY;
            int ai = lo, bi = lo;
            for (int c = lo; c < hi; ++c) {
                const float va = a[c], vb = b[c];
                d = fmaxf(d, fabsf(va - vb));
                if (va > am) am = va, ai = c;
                if (vb > b1) b2 = b1, b1 = vb, bi = c;
                else if (vb > b2) b2 = vb;
            }
            if (ai != bi) {
                if (b1 - b2 > p.near_tie) ++t_label;
                else ++t_tie;
            }
            t_head = fmaxf(t_head, d);
        }
        // the row's maximum over its four heads (the quad's lanes all have the same r)
        d = fmaxf(d, __shfl_xor(d, 1, 64));
        d = fmaxf(d, __shfl_xor(d, 2, 64));
        if (h == 0 && r < n) {
            t_over += d > p.tol;
            verify_max_row(t_max, t_row, d, (uint32_t)r);
        }
    }
    // the wave: lanes with the same head meet (distances 4 .. 32); (max, row) and the count of rows live on the lanes of head 0
    for (int off = 4; off < 64; off <<= 1) {
        t_head = fmaxf(t_head, __shfl_xor(t_head, off, 64));
        t_label += __shfl_xor(t_label, off, 64), t_tie += __shfl_xor(t_tie, off, 64), t_over += __shfl_xor(t_over, off, 64);
        const float om = __shfl_xor(t_max, off, 64);
        const uint32_t orow = __shfl_xor(t_row, off, 64);
        verify_max_row(t_max, t_row, om, orow);
    }
    if (lane < 4) {
        VerifyRecord &w = wave_rec[tid >> 6];
        w.head_max[lane] = t_head, w.label[lane] = t_label, w.tie[lane] = t_tie;
        if (lane == 0) w.max_abs = t_max, w.worst_row = t_row, w.rows_over = t_over;
    }
    __syncthreads();
    if (tid == 0) {
        VerifyRecord o = wave_rec[0];
        for (int w = 1; w < kVerifyThreads / 64; ++w) {
            const VerifyRecord &v = wave_rec[w];
            verify_max_row(o.max_abs, o.worst_row, v.max_abs, v.worst_row);
            o.rows_over += v.rows_over;
            for (int k = 0; k < 4; ++k) o.head_max[k] = fmaxf(o.head_max[k], v.head_max[k]), o.label[k] += v.label[k], o.tie[k] += v.tie[k];
        }
        o.n = 0;
        p.part[blockIdx.x] = o;
    }
}

// one wave: the partials of n_parts workgroups -> the batch's record
__global__ __launch_bounds__(64) C3_VERIFY_TEXT void rows_compare_final_kernel(const VerifyRecord *part, int n_parts, const uint32_t *kept, int batch, VerifyRecord *out) {
    const int lane = threadIdx.x;
    float mx = 0.f, hm[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t row = 0xffffffffu, over = 0, lab[4] = {0, 0, 0, 0}, tie[4] = {0, 0, 0, 0};
    for (int i = lane; i < n_parts; i += 64) {
        const VerifyRecord v = part[i];
        verify_max_row(mx, row, v.max_abs, v.worst_row);
        over += v.rows_over;
#pragma unroll
        for (int k = 0; k < 4; ++k) hm[k] = fmaxf(hm[k], v.head_max[k]), lab[k] += v.label[k], tie[k] += v.tie[k];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(mx, off, 64);
        const uint32_t orow = __shfl_xor(row, off, 64);
        verify_max_row(mx, row, om, orow);
        over += __shfl_xor(over, off, 64);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            hm[k] = fmaxf(hm[k], __shfl_xor(hm[k], off, 64)), lab[k] += __shfl_xor(lab[k], off, 64), tie[k] += __shfl_xor(tie[k], off, 64);
    }
    if (lane == 0) {
        VerifyRecord o;
        o.max_abs = mx, o.worst_row = row == 0xffffffffu ? 0u : row, o.rows_over = over;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.head_max[k] = hm[k], o.label[k] = lab[k], o.tie[k] = tie[k];
        o.n = kept ? min(*kept, (uint32_t)batch) : (uint32_t)batch;
        *out = o;
    }
}

// ------------------------------------------------------------------------------------------ layer records (c3_model_set_verify_layers)
// "Where" behind verify mode's "do my rows differ": per layer of a verified batch the output of the product form, a, against the output of
// the fp32 form, b, both in the checkpoint's units (the channel powers of two of the equalisation undone: the values c3_debug_tap_fetch
// returns).  Per layer and batch: max |a - b| (fp32), max |b|, max |a|, the lowest (window, index) that reaches max |a - b| -- index: the flat
// index inside the window, NHWC / (bin, c) / (t, feature) -- and the windows compared.  A value that is not finite counts as +inf: it must not
// vanish in an fmaxf.
//   layer_compare_kernel        streaming: a thread takes 8 consecutive channels per step -- a as plane slabs ([hi 64 x fp16 | lo 64 x fp16] per
//                               64 channels of a pixel row: one 16-byte hi piece, one lo piece) or as fp32 (two quads), b as two fp32 quads --
//                               and keeps its running (max, lowest position); butterfly over the wave, the four waves through LDS, one partial
//                               per workgroup.  One launch per layer and micro-batch, behind the fp32 form's launch of that layer
//   layer_compare_final_kernel  one wave per layer: the partials of all its launches -> the batch's record of that layer
// No atomics; maxima and the lexicographic (larger |d|, lower position) only: the record depends neither on the grid nor on scheduling.
constexpr int kLayerThreads = 256;
constexpr int kLayerMaxBlocks = 1024;      // partials of one launch
constexpr int kLayerMaxLayers = 11;        // full alignment: act0 .. act8, spp, l4_out; pileup: lstm1_out, gx2, lstm2_out, l4_out
constexpr size_t kLayerRecordsBytes = 512;  // the section of a staged batch: kLayerMaxLayers records, rounded up to a multiple of 256

struct LayerRecord {  // 8 words: a workgroup's partial, and a layer's record as c3_predict_wait reads it
    float max_abs, ref_max, test_max;
    uint32_t window, index;  // lowest position with |d| == max_abs (window 0xffffffff: no element yet)
    uint32_t windows;        // windows compared (the final record only)
    uint32_t compared;       // the final record only: 0 = the product form did not materialise the layer
    uint32_t pad;
};

struct LayerCompareParams {
    const void *a;         // the product form's output of this part: plane slabs (planes != 0) or fp32, [n][pw]
    const float *b;        // the fp32 form's, fp32 [n][pw]
    const int *exp;        // [1 << cshift << 3] channel c lives on the device times 2^exp[c], in a and in b alike; nullptr: none
    const uint32_t *kept;  // a candidate batch: the device word with the kept count; else nullptr
    LayerRecord *part;     // [gridDim.x]
    uint32_t pw8;          // values per window / 8
    int cshift;            // log2(channels / 8) of a plane tensor or one with exponents
    int planes;
    uint32_t first, n;     // this part: windows [first, first + n) of the batch
    uint32_t batch;
};

__device__ __forceinline__ float layer_abs(float v) {  // |v|, +inf for anything not finite
    v = fabsf(v);
    return v <= 3.402823466e+38f ? v : INFINITY;
}
__device__ __forceinline__ void layer_max_pos(float &m, uint32_t &w, uint32_t &i, float om, uint32_t ow, uint32_t oi) {
    if (om > m || (om == m && (ow < w || (ow == w && oi < i)))) m = om, w = ow, i = oi;
}

typedef _Float16 layer_half8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(kLayerThreads) C3_VERIFY_TEXT void layer_compare_kernel(LayerCompareParams p) {
    __shared__ LayerRecord wave_rec[kLayerThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    // windows of this part below the kept count (a dense batch: all of them)
    const uint32_t limit = p.kept ? min(*p.kept, p.batch) : p.batch;
    const uint32_t n = limit > p.first ? min(p.n, limit - p.first) : 0u;
    const uint32_t groups = n * p.pw8;  // of 8 values (host: n * pw < 2^32)
    const uint32_t cmask = (1u << p.cshift) - 1u;
    float t_max = 0.f, t_ref = 0.f, t_test = 0.f;
    uint32_t t_win = 0xffffffffu, t_idx = 0xffffffffu;
    for (uint32_t g = blockIdx.x * kLayerThreads + tid; g < groups; g += gridDim.x * kLayerThreads) {  // ascending per thread
        const uint32_t w = g / p.pw8, i0 = (g - w * p.pw8) * 8u, c0 = (g & cmask) * 8u;
        float va[8], vb[8];
        const float4 b0 = *reinterpret_cast<const float4 *>(p.b + (size_t)g * 8), b1 = *reinterpret_cast<const float4 *>(p.b + (size_t)g * 8 + 4);
        vb[0] = b0.x, vb[1] = b0.y, vb[2] = b0.z, vb[3] = b0.w, vb[4] = b1.x, vb[5] = b1.y, vb[6] = b1.z, vb[7] = b1.w;
        if (p.planes) {
            // pixel row r = g >> cshift holds channels / 64 slabs of 128 halves: the hi pieces of 64 channels, then their lo pieces
            const _Float16 *row = reinterpret_cast<const _Float16 *>(p.a) + ((size_t)(g >> p.cshift) << (p.cshift + 4)) + (c0 >> 6) * 128 + (c0 & 63);
            const layer_half8 hi = *reinterpret_cast<const layer_half8 *>(row), lo = *reinterpret_cast<const layer_half8 *>(row + 64);
#pragma unroll
            for (int k = 0; k < 8; ++k) va[k] = (float)hi[k] + (float)lo[k];
        } else {
            const float *a = reinterpret_cast<const float *>(p.a) + (size_t)g * 8;
            const float4 a0 = *reinterpret_cast<const float4 *>(a), a1 = *reinterpret_cast<const float4 *>(a + 4);
            va[0] = a0.x, va[1] = a0.y, va[2] = a0.z, va[3] = a0.w, va[4] = a1.x, va[5] = a1.y, va[6] = a1.z, va[7] = a1.w;
        }
        if (p.exp) {
            const int4 e0 = *reinterpret_cast<const int4 *>(p.exp + c0), e1 = *reinterpret_cast<const int4 *>(p.exp + c0 + 4);
            const int e[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) va[k] = ldexpf(va[k], -e[k]), vb[k] = ldexpf(vb[k], -e[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float d = layer_abs(va[k] - vb[k]);
            if (d > t_max || t_win == 0xffffffffu) t_max = d, t_win = w, t_idx = i0 + k;
            t_ref = fmaxf(t_ref, layer_abs(vb[k])), t_test = fmaxf(t_test, layer_abs(va[k]));
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(t_max, off, 64);
        const uint32_t ow = __shfl_xor(t_win, off, 64), oi = __shfl_xor(t_idx, off, 64);
        layer_max_pos(t_max, t_win, t_idx, om, ow, oi);
        t_ref = fmaxf(t_ref, __shfl_xor(t_ref, off, 64)), t_test = fmaxf(t_test, __shfl_xor(t_test, off, 64));
    }
    if (lane == 0) {
        LayerRecord &r = wave_rec[tid >> 6];
        r.max_abs = t_max, r.ref_max = t_ref, r.test_max = t_test, r.window = t_win, r.index = t_idx;
    }
    __syncthreads();
    if (tid == 0) {
        LayerRecord o = wave_rec[0];
        for (int w = 1; w < kLayerThreads / 64; ++w) {
            const LayerRecord &v = wave_rec[w];
            layer_max_pos(o.max_abs, o.window, o.index, v.max_abs, v.window, v.index);
            o.ref_max = fmaxf(o.ref_max, v.ref_max), o.test_max = fmaxf(o.test_max, v.test_max);
        }
        if (o.window != 0xffffffffu) o.window += p.first;  // the window's number in the batch
        o.windows = 0, o.compared = 1, o.pad = 0;
        p.part[blockIdx.x] = o;
    }
}

struct LayerFinalParams {
    const LayerRecord *part;  // layer k's partials: [part_at[k], part_at[k] + n_parts[k])
    const uint32_t *kept;
    LayerRecord *out;         // [gridDim.x]
    int batch;
    int part_at[kLayerMaxLayers];
    int n_parts[kLayerMaxLayers];  // 0: the product form did not materialise layer k
};

// one wave per layer: its partials -> its record of the batch
__global__ __launch_bounds__(64) C3_VERIFY_TEXT void layer_compare_final_kernel(LayerFinalParams p) {
    const int lane = threadIdx.x, k = blockIdx.x, np = p.n_parts[k];
    const LayerRecord *part = p.part + p.part_at[k];
    float mx = 0.f, ref = 0.f, test = 0.f;
    uint32_t win = 0xffffffffu, idx = 0xffffffffu;
    for (int i = lane; i < np; i += 64) {
        const LayerRecord v = part[i];
        layer_max_pos(mx, win, idx, v.max_abs, v.window, v.index);
        ref = fmaxf(ref, v.ref_max), test = fmaxf(test, v.test_max);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(mx, off, 64);
        const uint32_t ow = __shfl_xor(win, off, 64), oi = __shfl_xor(idx, off, 64);
        layer_max_pos(mx, win, idx, om, ow, oi);
        ref = fmaxf(ref, __shfl_xor(ref, off, 64)), test = fmaxf(test, __shfl_xor(test, off, 64));
    }
    if (lane == 0) {
        LayerRecord o;
        o.max_abs = mx, o.ref_max = ref, o.test_max = test;
        o.window = win == 0xffffffffu ? 0u : win, o.index = win == 0xffffffffu ? 0u : idx;
        o.windows = np == 0 ? 0u : p.kept ? min(*p.kept, (uint32_t)p.batch) : (uint32_t)p.batch;
        o.compared = np != 0, o.pad = 0;
        p.out[k] = o;
    }
}

}  // namespace c3
