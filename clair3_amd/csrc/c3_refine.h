// c3_refine.h -- refine mode (c3_model_set_refine): the windows of a batch whose label hangs on a near-tie are found on the
// device behind the product pass and answered by the exact form (c3_exact.h); every other row stays the product row, bit for bit.  The rule in
// numpy: synthetic.refine_gaps / refine_select.
//
// THE rule (include/c3hip.h, the numpy rule and the kernels below cite this block; tests/test_refine.py holds the two together):
//   head gap      per head h (columns (0,21) (21,24) (24,57) (57,90), limited to nout): g_h = b1 - b2 in float32, b1 the largest and b2 the
//                 second-largest value of the head, 0 when the maximum occurs twice -- the gap of c3_verify.h and of the census.  A head that
//                 holds a NaN has a NaN gap; a head the row does not have has none (+inf)
//   decoder gap   only for rows that carry decoder columns (stride > nout; c3_decode.h): for every reference base b of A, C, G, T that does NOT
//                 take the early exit (bit b of column 22) the top-2 gap, by the same rule, among the ten class maxima: column 9 + b (homo_Ref
//                 for that base) and columns 0 .. 8.  The decoder gap is the minimum over those bases; all four on the early exit: none (+inf)
//   selection     a window is selected iff any of its gaps is <= gap, compared in float32.  A NaN gap selects nothing (every comparison with
//                 it fails): a non-finite row is the range guard's business
//   minimum gap   of a window: the minimum of its gaps that are not NaN (fminf), NaN when all of them are
// Stated limit: near-ties INSIDE one outcome class list are caught only through the head gaps they are products of.
//
// Launches, all on the batch's stream, no atomics in the selection (every combination is an integer sum, a minimum or a prefix in window
// order: the list and the record do not depend on scheduling):
//   rows_gap_kernel         four lanes per window -- lane h takes head h and reference base h --, 64 windows per workgroup: every window's
//                           minimum gap and selection bits (bit h: head h, bit 4: decoder), one partial per workgroup
//   refine_compact_kernel   one wave per workgroup of the first launch: its offset is the sum of the counts before it, its windows' places
//                           follow from a ballot; the selected indices in ascending window order.  The last workgroup adds the partials up
//                           into the batch's record
//   refine_gather_kernel    the selected windows of the staged image, whatever their byte address, into a contiguous buffer
//   refine_scatter_kernel   the refined rows back at their indices, probabilities and decoder columns; counts the windows in which the
//                           arg-max of a head changed and keeps the largest |refined - product| (two integer atomics: a sum and a maximum of
//                           bit patterns of floats >= 0)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

constexpr int kRefineThreads = 256;           // 64 windows per workgroup
constexpr int kRefineWindows = kRefineThreads / 4;
constexpr int64_t kRefineMaxBatch = (int64_t)1 << 22;  // windows of one batch the selection takes (65536 workgroups: the offsets are summed per workgroup)
constexpr size_t kRefineRecordBytes = 256;    // the record at the front of a staged batch's refine section, int32[batch] indices behind it

struct RefinePart {  // a workgroup's partial
    uint32_t selected, head[4], decoder;
    float min_gap[4];
};
struct RefineRecord {  // the batch's record as c3_predict_wait reads it
    uint32_t windows, selected, head[4], decoder;
    float min_gap[4];  // per head over the batch's windows, NaN gaps left out (+inf: none)
    // ... written by refine_scatter_kernel (zero behind refine_compact_kernel)
    uint32_t changed;        // refined windows in which the arg-max of a head changed
    uint32_t max_diff_bits;  // bit pattern of max |refined - product| over the refined probabilities
    uint32_t pad[51];
};
static_assert(sizeof(RefineRecord) == kRefineRecordBytes, "RefineRecord fills its section");

struct RefineGapParams {
    const float *rows;  // [batch][stride]: nout probabilities, kDecodeCols decoder columns behind them when stride > nout
    float *min_gap;     // [batch]
    uint8_t *bits;      // [batch]
    RefinePart *part;   // [gridDim.x]
    int stride, nout, batch;
    float gap;
};

#define C3_REFINE_TEXT __attribute__((section(".c3_refine_text")))  // behind `.c3_census_text`: no other kernel moves

// the top-2 gap of n values v(0) .. v(n - 1) by the rule above
template <class F>
__device__ __forceinline__ float refine_top2_gap(int n, F v) {
    float b1 = -INFINITY, b2 = -INFINITY;
    bool nan = false;
    for (int c = 0; c < n; ++c) {
        const float x = v(c);
        nan |= x != x;
        if (x > b1) b2 = b1, b1 = x;
        else if (x > b2) b2 = x;
    }
    return nan ? NAN : b1 - b2;
}

__global__ __launch_bounds__(kRefineThreads) C3_REFINE_TEXT void rows_gap_kernel(RefineGapParams p) {
    __shared__ RefinePart wave_part[kRefineThreads / 64];
    const int tid = threadIdx.x, h = tid & 3, lane = tid & 63;
    const int r = blockIdx.x * kRefineWindows + (tid >> 2);
    const int lo = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
    const int hi = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
    float hg = INFINITY, dg = INFINITY;
    if (r < p.batch) {
        const float *row = p.rows + (int64_t)r * p.stride;
        if (lo < hi) hg = refine_top2_gap(hi - lo, [&](int c) { return row[lo + c]; });
        if (p.stride > p.nout) {
            const float *cols = row + p.nout;
            if (!((unsigned)cols[22] >> h & 1u)) dg = refine_top2_gap(10, [&](int c) { return c == 0 ? cols[9 + h] : cols[c - 1]; });
        }
    }
    // (every lane reaches the ballots; a lane without a window holds +inf twice and selects nothing)
    const unsigned long long bh = __ballot(hg <= p.gap), bd = __ballot(dg <= p.gap);
    const int quad = lane & ~3;
    const unsigned hbits = (unsigned)(bh >> quad) & 15u, dsel = ((unsigned)(bd >> quad) & 15u) != 0;
    float mg = fminf(hg, dg);
    mg = fminf(mg, __shfl_xor(mg, 1, 64));
    mg = fminf(mg, __shfl_xor(mg, 2, 64));
    if (h == 0 && r < p.batch) p.min_gap[r] = mg, p.bits[r] = (uint8_t)(hbits | dsel << 4);
    // the wave: counts from the ballots, the heads' minima over the lanes of the same head (xor distances 4 .. 32)
    float hm = hg;
    for (int off = 4; off < 64; off <<= 1) hm = fminf(hm, __shfl_xor(hm, off, 64));
    const unsigned long long first = 0x1111111111111111ull;  // the first lane of every quad
    const unsigned long long sel = __ballot(h == 0 && (hbits | dsel) != 0), dec = __ballot(h == 0 && dsel);
    if (lane < 4) {
        RefinePart &w = wave_part[tid >> 6];
        w.head[lane] = (uint32_t)__popcll(bh & first << lane), w.min_gap[lane] = hm;
        if (lane == 0) w.selected = (uint32_t)__popcll(sel), w.decoder = (uint32_t)__popcll(dec);
    }
    __syncthreads();
    if (tid == 0) {
        RefinePart o = wave_part[0];
        for (int w = 1; w < kRefineThreads / 64; ++w) {
            const RefinePart &v = wave_part[w];
            o.selected += v.selected, o.decoder += v.decoder;
            for (int k = 0; k < 4; ++k) o.head[k] += v.head[k], o.min_gap[k] = fminf(o.min_gap[k], v.min_gap[k]);
        }
        p.part[blockIdx.x] = o;
    }
}

// one wave per workgroup of rows_gap_kernel (the same grid): index[] holds the selected windows in ascending order, *rec the batch's record
__global__ __launch_bounds__(64) C3_REFINE_TEXT void refine_compact_kernel(const uint8_t *bits, const RefinePart *part, int batch, int32_t *index,
                                                                           RefineRecord *rec) {
    const int lane = threadIdx.x, k = blockIdx.x;
    uint32_t base = 0;
    for (int i = lane; i < k; i += 64) base += part[i].selected;
    for (int off = 32; off > 0; off >>= 1) base += __shfl_xor(base, off, 64);
    const int r = k * kRefineWindows + lane;
    const bool sel = r < batch && bits[r] != 0;
    const unsigned long long mask = __ballot(sel);
    if (sel) index[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = r;
    if (k != (int)gridDim.x - 1) return;
    // the last workgroup: every partial -> the record
    uint32_t cnt[5] = {0, 0, 0, 0, 0};
    float mn[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    for (int i = lane; i <= k; i += 64) {
        const RefinePart v = part[i];
        cnt[4] += v.decoder;
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt[j] += v.head[j], mn[j] = fminf(mn[j], v.min_gap[j]);
    }
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 5; ++j) cnt[j] += __shfl_xor(cnt[j], off, 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) mn[j] = fminf(mn[j], __shfl_xor(mn[j], off, 64));
    }
    if (lane == 0) {
        RefineRecord o = RefineRecord{};
        o.windows = (uint32_t)batch, o.selected = base + (uint32_t)__popcll(mask), o.decoder = cnt[4];
        for (int j = 0; j < 4; ++j) o.head[j] = cnt[j], o.min_gap[j] = mn[j];
        *rec = o;
    }
}

// workgroup j: window index[j] of the image (windows of wbytes bytes back to back) -> window j of out, in pieces of V bytes (V = 8 needs
// wbytes % 8 == 0 and both buffers 8-byte aligned; V = 1 takes any: the 9-channel full-alignment window has 26433 bytes)
template <int V>
__global__ __launch_bounds__(256) C3_REFINE_TEXT void refine_gather_kernel(const char *image, const int32_t *index, char *out, int64_t wbytes) {
    const char *src = image + (int64_t)index[blockIdx.x] * wbytes;
    char *dst = out + (int64_t)blockIdx.x * wbytes;
    if constexpr (V == 8) {
        for (int64_t i = threadIdx.x; i < wbytes / 8; i += 256) reinterpret_cast<uint2 *>(dst)[i] = reinterpret_cast<const uint2 *>(src)[i];
    } else {
        for (int64_t i = threadIdx.x; i < wbytes; i += 256) dst[i] = src[i];
    }
}

struct RefineScatterParams {
    const float *refined;  // [n][stride]: the exact form's float32 rows of the selected windows, decoder columns filled in
    const int32_t *index;  // [n]
    float *rows;           // [batch][stride], rows index[j] are overwritten
    RefineRecord *rec;
    int stride, nout, n;
};
// four lanes per refined window: lane h compares and copies the columns of head h, then every fourth decoder column
__global__ __launch_bounds__(kRefineThreads) C3_REFINE_TEXT void refine_scatter_kernel(RefineScatterParams p) {
    const int tid = threadIdx.x, h = tid & 3, lane = tid & 63;
    const int j = blockIdx.x * kRefineWindows + (tid >> 2);
    const int lo = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
    const int hi = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
    float d = 0.f;
    bool moved = false;
    if (j < p.n) {
        const float *b = p.refined + (int64_t)j * p.stride;
        float *a = p.rows + (int64_t)p.index[j] * p.stride;
        float am = -INFINITY, bm = -INFINITY;
        int ai = lo, bi = lo;
        for (int c = lo; c < hi; ++c) {  // (the arg-max rule of c3_verify.h: the first maximum, a NaN never)
            const float va = a[c], vb = b[c];
            d = fmaxf(d, fabsf(va - vb));
            if (va > am) am = va, ai = c;
            if (vb > bm) bm = vb, bi = c;
            a[c] = vb;
        }
        moved = ai != bi;
        for (int c = p.nout + h; c < p.stride; c += 4) a[c] = b[c];
    }
    const unsigned long long mv = __ballot(moved);
    const unsigned changed = ((unsigned)(mv >> (lane & ~3)) & 15u) != 0;
    const unsigned long long win = __ballot(h == 0 && changed);
    for (int off = 1; off < 64; off <<= 1) d = fmaxf(d, __shfl_xor(d, off, 64));
    if (lane == 0) {
        if (win) atomicAdd(&p.rec->changed, (uint32_t)__popcll(win));
        if (d > 0.f) atomicMax(&p.rec->max_diff_bits, __float_as_uint(d));
    }
}

static inline unsigned refine_blocks(int64_t n) { return (unsigned)((n + kRefineWindows - 1) / kRefineWindows); }
// the scratch of a selection over `batch` windows: the windows' minimum gaps, their bits, the workgroups' partials -- one allocation
struct RefineScratch {
    size_t gaps_at = 0, bits_at = 0, part_at = 0, bytes = 0;
    explicit RefineScratch(int64_t batch) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        bits_at = al((size_t)batch * sizeof(float)), part_at = al(bits_at + (size_t)batch);
        bytes = part_at + (size_t)refine_blocks(batch) * sizeof(RefinePart);
    }
};

}  // namespace c3
