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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

constexpr int kVerifyThreads = 256;     // 64 rows per workgroup and pass
constexpr int kVerifyMaxBlocks = 1024;  // partials of one batch (a larger batch: every workgroup takes several passes)
constexpr size_t kVerifyRecordBytes = 256;  // the record's section of a staged batch (a multiple of 256 like every section)

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

}  // namespace c3
