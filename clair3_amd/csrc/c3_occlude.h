// c3_occlude.h -- occlusion mode (c3_occlude, c3_occlude_rows, c3_occlude_reduce): which input channels and which columns a
// call leans on, for BOTH networks.  For every window of a call the device builds K variants from the window staged once -- the window with
// one channel set to zero, the window with one band of columns set to zero --, runs them through the unchanged forward pass beside the window
// itself and reduces their rows to one 144-byte record per window plus the complete map of drops.  An instrument like jackknife mode
// (c3_jackknife.h), whose machinery it follows: nothing is allocated, launched or planned unless one of the three entries is called.  The
// rule in numpy: synthetic.occlude_variants / occlude_records.
//
// THE definitions (include/c3hip.h, the numpy rule and the kernels below cite this block; tests/test_occlude.py holds them together).
// A window has P positions and C channels, the handle's geometry: full alignment (depth, P, C) int8, pileup (P, C) int8 or int32.  A call
// names `what` (C3_OCCLUDE_CHANNELS = 1, C3_OCCLUDE_BANDS = 2, both = 3) and `band` (1 <= band <= P, columns per band);
// nb = ceil(P / band), band k covers the columns [k * band, min(P, (k + 1) * band)).
//   variants        every window of the call has the same K = (C if channels) + (nb if bands) variants, in this order: group 0, when
//                   channels are asked for: variant c (0 <= c < C) is the window with channel c set to zero at every position, and in every
//                   read for full alignment; group 1, when bands are asked for: variant k (0 <= k < nb) is the window with every channel of
//                   band k's columns set to zero, in every read.  Everything else stays where it is: a full-alignment variant keeps the base
//                   window's run where row_first / the centring rule puts it -- a read is not removed, so nothing is laid out again.
//                   Window b's variants are the call's variants b * K .. b * K + K - 1.  A window without reads, or an all-zero window,
//                   still has K variants: all of them the zero window
//   arg-max         of a head: the first maximum by `>` from -inf on -- lowest index on ties, a NaN never, the head's first column when
//                   nothing exceeds -inf (the rule of c3_census.h, c3_refine.h and c3_jackknife.h).  Heads are columns (0,21) (21,24) (24,57)
//                   (57,90) limited to nout
//   variants        (the record's field) K
//   nonfinite       variants with a value among their first nout columns that is not finite
//   flips[g][h]     the variants of group g whose arg-max in head h differs from the base row's, non-finite variants included (0 for a head
//                   the model lacks, 0 for a group that was not asked for)
//   decision_flips  [g][r]: rows with decoder columns (stride > nout; c3_decode.h): the variants of group g whose decoder column 23 + r
//                   compares unequal (float !=) to the base row's, r = A C G T; rows without decoder columns: 0
//   drop            of variant j in head h: y[t] - v_j[t] in one float32 subtraction, t the base row's arg-max of the head (0 for a head the
//                   model lacks)
//   lean[g][h]      the index within group g (the channel c, or the band k) of the largest drop among the variants that are finite and whose
//                   drop is not a NaN (a NaN base row has none), the lowest index on ties; -1 when there is none or the group was not asked
//                   for.  lean_drop[g][h]: that drop (may be negative), 0 with lean -1; a zero that leans is +0
//   max_delta       max over the finite variants and the first nout columns of |v_j[c] - y[c]| in float32, differences that are NaN left
//                   out; 0 without any
//   the map         drops [batch][K][4] float32: the drop of every variant in every head -- the saliency profile over channels and columns;
//                   the record only summarises it
// Only integer counts, comparisons and single float32 subtractions: the record is exactly what the numpy rule gives on the same rows.
//
// Launches (the active lane's stream; no atomics, nothing depends on scheduling):
//   occlude_expand_kernel<V>         expand_rows_kernel (c3_expand.h) with a mask: one workgroup per dense full-alignment window to build
//   occlude_pileup_expand_kernel<T>  the staged (B, P, C) windows into the dense windows of a micro-batch, in a buffer of the lane
//   occlude_reduce_kernel            one wave per window, lanes striding over its K variants; counts are summed and maxima taken by a
//                                    butterfly on keys (jackknife_key of the drop, then lowest index)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

namespace c3 {

#define C3_OCCLUDE_TEXT __attribute__((section(".c3_occlude_text")))  // behind `.c3_subsample_text`: no other kernel moves

// one per dense window to build, filled by the host (occlude_fill_pass); workgroup-uniform in the kernels
struct OccludeEntry {
    int64_t src;      // byte offset of the window's staged input in the pass's: its first occupied row (full alignment), the window (pileup)
    int32_t first;    // full alignment: dense row the run starts at (pileup: 0)
    int32_t count;    // full alignment: source rows (pileup: 0)
    int32_t chan;     // >= 0: the channel to set to zero; -1: none
    int32_t col_lo;   // columns [col_lo, col_hi) to set to zero; empty: none
    int32_t col_hi;
    int32_t pad;
};
static_assert(sizeof(OccludeEntry) == 32, "OccludeEntry is 32 bytes");
static_assert(sizeof(c3_occlude_window) == 144, "c3_occlude_window is 144 bytes (include/c3hip.h, synthetic.OCCLUDE_DTYPE)");

struct OccludeExpandParams {
    const int8_t *in;         // the pass's staged input
    const OccludeEntry *tab;  // [B]
    void *out;                // [B] dense windows
    int B;
    int P, C;                     // positions, channels
    int row_bytes, window_bytes;  // full alignment: P * C, depth * row_bytes (pileup: unused)
};

// Where element i = i0 + k * step (k = 0, 1, ..) of a [..][P][C] array sits: its channel c = i % C and its column pos = (i / C) % P, kept by
// additions and two conditional subtractions per step -- the two divisions are made once per thread, none per element.
struct OccludeWalk {
    int c, pos, dc, dpos, C, P;
    __device__ __forceinline__ OccludeWalk(int i0, int step, int C_, int P_) : C(C_), P(P_) {
        c = i0 % C, pos = (i0 / C) % P, dc = step % C, dpos = (step / C) % P;
    }
    __device__ __forceinline__ void next() {
        c += dc;
        const int carry = c >= C ? 1 : 0;
        c -= carry ? C : 0;
        pos += dpos + carry;  // (< 2 P)
        pos -= pos >= P ? P : 0;
    }
};

// One workgroup per dense window, the entry workgroup-uniform.  As expand_rows_kernel, destination piece p is zero outside [lo, hi) =
// [first * rp, (first + count) * rp) and source piece p - lo inside; the mask then clears what the variant occludes.  Every destination byte
// is written exactly once -- a zero, a source byte or a masked source byte --, no memset, no atomics.
//   V = 8 (C == 8 only): an 8-byte piece is one (read, position) cell, a channel is a byte mask on the piece, a band a range of piece % P --
//         kept by OccludeWalk with one channel per cell.  (For an even C other than 8 a piece is not a cell: those go to the byte form.)
//   V = 1 (any other C, the dwell model's 297-byte rows): bytes, channel and column by OccludeWalk.
template <int V>
__global__ __launch_bounds__(kExpandThreads) C3_OCCLUDE_TEXT void occlude_expand_kernel(OccludeExpandParams p) {
    const int b = blockIdx.x;
    if (b >= p.B) return;
    const OccludeEntry e = p.tab[b];
    const int rp = p.row_bytes / V, n = p.window_bytes / V;
    const int lo = e.first * rp, hi = lo + e.count * rp;
    if constexpr (V == 8) {
        const uint2 *src = reinterpret_cast<const uint2 *>(p.in + e.src);
        uint2 *dst = reinterpret_cast<uint2 *>(static_cast<int8_t *>(p.out) + (int64_t)b * p.window_bytes);
        // the bytes of a cell that stay: all but channel `chan`
        const uint32_t keep_x = e.chan >= 0 && e.chan < 4 ? ~(0xffu << (8 * e.chan)) : 0xffffffffu;
        const uint32_t keep_y = e.chan >= 4 && e.chan < 8 ? ~(0xffu << (8 * (e.chan - 4))) : 0xffffffffu;
        OccludeWalk w(threadIdx.x, kExpandThreads, 1, p.P);
        for (int i = threadIdx.x; i < n; i += kExpandThreads, w.next()) {
            uint2 v = make_uint2(0u, 0u);
            if (i >= lo && i < hi && !(w.pos >= e.col_lo && w.pos < e.col_hi)) {
                v = src[i - lo];
                v.x &= keep_x, v.y &= keep_y;
            }
            dst[i] = v;
        }
    } else {
        const int8_t *src = p.in + e.src;
        int8_t *dst = static_cast<int8_t *>(p.out) + (int64_t)b * p.window_bytes;
        OccludeWalk w(threadIdx.x, kExpandThreads, p.C, p.P);
        for (int i = threadIdx.x; i < n; i += kExpandThreads, w.next()) {
            int8_t v = 0;
            if (i >= lo && i < hi && w.c != e.chan && !(w.pos >= e.col_lo && w.pos < e.col_hi)) v = src[i - lo];
            dst[i] = v;
        }
    }
}

// One workgroup per dense pileup window of P * C elements of T, read and written element by element: a 594-byte int8 window is only 2-byte
// aligned, and nothing more is assumed.  Every destination element is written exactly once.
template <typename T>
__global__ __launch_bounds__(kExpandThreads) C3_OCCLUDE_TEXT void occlude_pileup_expand_kernel(OccludeExpandParams p) {
    const int b = blockIdx.x;
    if (b >= p.B) return;
    const OccludeEntry e = p.tab[b];
    const int n = p.P * p.C;
    const T *src = reinterpret_cast<const T *>(p.in + e.src);
    T *dst = static_cast<T *>(p.out) + (int64_t)b * n;
    OccludeWalk w(threadIdx.x, kExpandThreads, p.C, p.P);
    for (int i = threadIdx.x; i < n; i += kExpandThreads, w.next()) {
        T v = 0;
        if (w.c != e.chan && !(w.pos >= e.col_lo && w.pos < e.col_hi)) v = src[i];
        dst[i] = v;
    }
}

struct OccludeReduceParams {
    const float *base;       // [batch][stride]: the windows' own rows
    const float *variants;   // [batch][K][stride]: the variants' rows, window after window, group 0 then group 1
    c3_occlude_window *out;  // [batch]
    float *drops;            // [batch][K][4], or null
    int stride, nout, batch;
    int channels, bands;  // the sizes of the two groups; K = channels + bands
};

// One wave per window, lanes striding over its K variants (K <= 51 for the shipped geometries: one variant per lane; the stride loop stays
// for other geometries).  Every lane accumulates into the group its variant belongs to; the butterfly sums the counts and takes the maxima
// of (jackknife_key of the drop) << 32 | ~index, 0 = none: the largest drop, then the lowest index.  No atomics.
__global__ __launch_bounds__(64) C3_OCCLUDE_TEXT void occlude_reduce_kernel(OccludeReduceParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= p.batch) return;
    const float *y = p.base + (int64_t)b * p.stride;
    const int K = p.channels + p.bands;
    const int64_t at = (int64_t)b * K;
    const bool cols = p.stride > p.nout;
    // the base row's arg-maxima (every lane: the loads are wave-uniform)
    int t[4], lo[4], hi[4];
    float yt[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        lo[h] = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
        hi[h] = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
        t[h] = lo[h], yt[h] = 0.f;
        if (lo[h] >= hi[h]) continue;
        float best = -INFINITY;
        for (int c = lo[h]; c < hi[h]; ++c)
            if (y[c] > best) best = y[c], t[h] = c;
        yt[h] = y[t[h]];
    }
    uint32_t nonfinite = 0, delta = 0;  // delta: bits of a float >= 0
    uint32_t flips[2][4] = {}, dflips[2][4] = {};
    unsigned long long lean[2][4] = {};  // key of the drop << 32 | ~index within the group; 0: none
    for (int j = lane; j < K; j += 64) {
        const float *v = p.variants + (at + j) * p.stride;
        const bool g1 = j >= p.channels;  // the variant's group ...
        const uint32_t idx = (uint32_t)(g1 ? j - p.channels : j);  // ... and its index within it
        bool finite = true;
        float d = 0.f;
        int am[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            am[h] = lo[h];
            float best = -INFINITY;
            for (int c = lo[h]; c < hi[h]; ++c) {
                const float x = v[c];
                finite &= (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
                const float a = fabsf(x - y[c]);
                if (a > d) d = a;
                if (x > best) best = x, am[h] = c;
            }
        }
        nonfinite += !finite;
        if (finite) delta = max(delta, __float_as_uint(d));
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const bool has = lo[h] < hi[h];
            const float drop = has ? yt[h] - v[t[h]] : 0.f;
            if (p.drops) p.drops[(at + j) * 4 + h] = drop;
            if (!has) continue;
            const uint32_t flip = am[h] != t[h];
            flips[0][h] += g1 ? 0u : flip, flips[1][h] += g1 ? flip : 0u;
            if (finite && drop == drop) {
                const unsigned long long key = (unsigned long long)jackknife_key(drop) << 32 | (uint32_t)~idx;
                const unsigned long long k0 = g1 ? 0ull : key, k1 = g1 ? key : 0ull;
                lean[0][h] = k0 > lean[0][h] ? k0 : lean[0][h], lean[1][h] = k1 > lean[1][h] ? k1 : lean[1][h];
            }
        }
        if (cols) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t df = v[p.nout + 23 + r] != y[p.nout + 23 + r];
                dflips[0][r] += g1 ? 0u : df, dflips[1][r] += g1 ? df : 0u;
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        nonfinite += __shfl_xor(nonfinite, off, 64);
        delta = max(delta, (uint32_t)__shfl_xor(delta, off, 64));
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                flips[g][h] += __shfl_xor(flips[g][h], off, 64), dflips[g][h] += __shfl_xor(dflips[g][h], off, 64);
                const unsigned long long o = __shfl_xor(lean[g][h], off, 64);
                lean[g][h] = o > lean[g][h] ? o : lean[g][h];
            }
    }
    if (lane != 0) return;
    c3_occlude_window r;
    r.variants = K, r.nonfinite = (int32_t)nonfinite;
    for (int g = 0; g < 2; ++g)
        for (int h = 0; h < 4; ++h) {
            r.flips[g][h] = (int32_t)flips[g][h], r.decision_flips[g][h] = (int32_t)dflips[g][h];
            r.lean[g][h] = lean[g][h] ? (int32_t)~(uint32_t)lean[g][h] : -1;
            r.lean_drop[g][h] = lean[g][h] ? jackknife_unkey((uint32_t)(lean[g][h] >> 32)) : 0.f;
        }
    r.max_delta = __uint_as_float(delta), r.reserved = 0;
    p.out[b] = r;
}

// ------------------------------------------------------------------------------------------ the host's plan (plain host code: tests/host/
// occlude_host_check.cpp drives it against buffers of exactly these sizes)
// what a call asks for, worked out once: the two groups' sizes for the handle's geometry
struct OccludePlan {
    int P = 0, C = 0, what = 0, band = 0;
    int channels = 0, bands = 0;  // group 0: C or 0; group 1: nb = ceil(P / band) or 0
    int K() const { return channels + bands; }
    OccludePlan() {}
    OccludePlan(int P_, int C_, int what_, int band_) : P(P_), C(C_), what(what_), band(band_) {
        channels = what & C3_OCCLUDE_CHANNELS ? C : 0;
        bands = what & C3_OCCLUDE_BANDS ? (P + band - 1) / band : 0;
    }
};
// A call is cut into passes of `chunk` windows (0: one pass); a window's variants never straddle a pass.
struct OccludePass {
    int64_t w0 = 0, windows = 0;     // the windows [w0, w0 + windows) of the call
    int64_t unit0 = 0, units = 0;    // their staged units in the caller's input: occupied rows (full alignment), windows (pileup)
    int64_t var0 = 0, variants = 0;  // their variants among the call's: [var0, var0 + variants), K a window
    int64_t dense() const { return windows + variants; }  // dense windows the pass builds: base windows first, then every variant
};
// env C3HIP_OCCLUDE_CHUNK: windows per pass, 0 = never cut; default 64 full-alignment windows (jackknife mode's pass), 256 pileup windows
// (256 * 52 dense windows stay below the pileup micro-batch of 16384)
static inline int64_t occlude_chunk_env(int kind) {
    const int64_t dflt = kind == C3_KIND_PILEUP ? 256 : 64;
    const char *e = getenv("C3HIP_OCCLUDE_CHUNK");
    const long long v = e ? atoll(e) : dflt;
    return v < 0 ? dflt : (int64_t)v;
}
// count: the windows' occupied rows (full alignment), or null: one unit a window (pileup)
static inline std::vector<OccludePass> occlude_cut(const int32_t *count, int64_t batch, int64_t chunk, int K) {
    std::vector<OccludePass> out;
    int64_t unit = 0;
    for (int64_t w = 0; w < batch;) {
        OccludePass ps;
        ps.w0 = w, ps.windows = chunk > 0 ? std::min(chunk, batch - w) : batch - w, ps.unit0 = unit, ps.var0 = w * K;
        for (int64_t i = 0; i < ps.windows; ++i) ps.units += count ? count[w + i] : 1;
        ps.variants = ps.windows * K;
        out.push_back(ps);
        w += ps.windows, unit += ps.units;
    }
    return out;
}
// where a pass's sections sit in the handle's occlusion buffer (every section from a multiple of 256 bytes): the staged input, the table,
// the rows of the dense windows, the records with the pass's copy of the range flag behind them, the drops
struct OccludeLayout {
    size_t in_at = 0, tab_at = 0, tab_end = 0;                          // staged
    size_t y_at = 0, rec_at = 0, flag_at = 0, drops_at = 0, bytes = 0;  // written by the device
    OccludeLayout(const OccludePass &ps, size_t unit_bytes, int row_floats, bool drops) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        tab_at = al((size_t)ps.units * unit_bytes);
        tab_end = tab_at + (size_t)ps.dense() * sizeof(OccludeEntry);
        y_at = al(tab_end);
        rec_at = al(y_at + (size_t)ps.dense() * row_floats * sizeof(float));
        flag_at = rec_at + (size_t)ps.windows * sizeof(c3_occlude_window);  // (144-byte records: a multiple of 4)
        drops_at = al(flag_at + 4);
        bytes = drops_at + (drops ? (size_t)ps.variants * 4 * sizeof(float) : 0);
    }
    size_t tab_bytes() const { return tab_end - tab_at; }
};
// the table of a pass as it is staged, `tab` of ps.dense() entries: the base entries first (no mask), then every window's K variants in
// window order and variant order -- channels 0 .. C - 1, then bands 0 .. nb - 1.  first[] / count[] are the call's, checked by the entry
// (full alignment), or null (pileup: one unit of unit_bytes a window)
static inline void occlude_fill_pass(OccludeEntry *tab, const OccludePass &ps, const OccludePlan &plan, const int32_t *first, const int32_t *count,
                                     size_t unit_bytes) {
    const int K = plan.K();
    int64_t unit = 0;
    for (int64_t i = 0; i < ps.windows; ++i) {
        const int32_t n = count ? count[ps.w0 + i] : 0, f = first ? first[ps.w0 + i] : 0;
        const OccludeEntry e{(int64_t)(unit * (int64_t)unit_bytes), f, n, -1, 0, 0, 0};
        tab[i] = e;
        OccludeEntry *v = tab + ps.windows + i * K;
        for (int c = 0; c < plan.channels; ++c) v[c] = e, v[c].chan = c;
        for (int k = 0; k < plan.bands; ++k)
            v[plan.channels + k] = e, v[plan.channels + k].col_lo = k * plan.band, v[plan.channels + k].col_hi = std::min(plan.P, (k + 1) * plan.band);
        unit += count ? n : 1;
    }
}

}  // namespace c3

// ------------------------------------------------------------------------------------------ the entries (include/c3hip.h)
// the handle's occlusion buffer: a pass's staged input, its table, the rows of its dense windows, the records, the drops; grown, never shrunk
static int ensure_occlude_buf(c3_model *m, size_t bytes) {
    if (m->occlude_bytes >= bytes) return 0;
    HIP_TRY(hipDeviceSynchronize());
    if (m->occlude_dev) (void)hipFree(m->occlude_dev);
    m->occlude_dev = nullptr, m->occlude_bytes = 0;
    HIP_TRY(hipMalloc(&m->occlude_dev, bytes));
    m->occlude_bytes = bytes;
    return 0;
}

// the active lane's buffer of dense pileup windows that occlude_pileup_expand_kernel builds, sized like the lane's buffer of rescaled
// windows (ensure_rescale_buf): as many int32 windows as its workspace holds; allocated on first use, grown, freed with the workspace
static int ensure_occlude_window_buf(c3_model *m) {
    Lane &L = lane(m);
    if (L.xo && L.xo_cap >= L.cap) return 0;
    HIP_TRY(hipDeviceSynchronize());
    if (L.xo) (void)hipFree(L.xo);
    L.xo = nullptr, L.xo_cap = 0;
    HIP_TRY(hipMalloc(&L.xo, std::max<size_t>((size_t)L.cap * m->positions * m->C * sizeof(int32_t), 256)));
    L.xo_cap = L.cap;
    return 0;
}

static int occlude_reduce_launch(hipStream_t s, const OccludeReduceParams &rp, JackknifeTimer *timer = nullptr) {
    if (rp.batch <= 0) return 0;
    if (timer) timer->mark(s);
    hipLaunchKernelGGL(occlude_reduce_kernel, dim3((unsigned)rp.batch), dim3(64), 0, s, rp);
    HIP_TRY(hipGetLastError());
    if (timer) timer->mark(s);
    return 0;
}

// the dense windows of a pass, micro-batch by micro-batch through the forms the handle is on, their rows at y (row stride m->row): the
// micro-batch loop of jackknife_forward; int8 and int32 pileup windows stay on their own kernels, as in forward_device
static int occlude_forward(c3_model *m, hipStream_t s, const int8_t *in, const OccludeEntry *tab, int64_t total, int x_dtype, float *y,
                           JackknifeTimer &timer) {
    TRY(ensure_workspace(m, total));
    const bool fa = m->kind == C3_KIND_FULL_ALIGNMENT;
    if (fa) TRY(ensure_expand_buf(m));
    else TRY(ensure_occlude_window_buf(m));
    Lane &L = lane(m);
    const int64_t wbytes = c3_model_window_bytes(m, x_dtype);
    for (int64_t off = 0; off < total; off += L.cap) {
        const int64_t n = std::min<int64_t>(L.cap, total - off);
        const OccludeExpandParams ep{in, tab + off, fa ? (void *)L.xe : L.xo, (int)n, m->positions, m->C, m->positions * m->C, (int)wbytes};
        const dim3 grid((unsigned)n), block(kExpandThreads);
        timer.mark(s);
        if (fa && m->C == 8) hipLaunchKernelGGL(occlude_expand_kernel<8>, grid, block, 0, s, ep);  // (a piece is a cell only when C == 8)
        else if (fa) hipLaunchKernelGGL(occlude_expand_kernel<1>, grid, block, 0, s, ep);
        else if (x_dtype == C3_DTYPE_I8) hipLaunchKernelGGL(occlude_pileup_expand_kernel<int8_t>, grid, block, 0, s, ep);
        else hipLaunchKernelGGL(occlude_pileup_expand_kernel<int32_t>, grid, block, 0, s, ep);
        HIP_TRY(hipGetLastError());
        timer.mark(s);
        float *yp = y + off * m->row;
        if (fa) TRY(run_fa(m, s, L.xe, n, yp));
        else if (x_dtype == C3_DTYPE_I8) TRY(run_pileup_t<int8_t>(m, s, (const int8_t *)L.xo, n, yp));
        else TRY(run_pileup_t<int32_t>(m, s, (const int32_t *)L.xo, n, yp));
        L.last_n = n;
    }
    return 0;
}

// what the two entries that run the network refuse before anything is queued
static int occlude_handle(c3_model *m, const char *who, int what, int band) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("%s: a prediction is in flight: call c3_predict_wait first", who);
    if (m->answer_exact) return fail("%s: the handle answers from the exact form: c3_model_set_answer(m, C3_ANSWER_PRODUCT) first", who);
    if (!m->loaded) return fail("model has no weights: call c3_model_load first");
    if (what < 1 || what > 3) return fail("%s: unknown `what` %d (C3_OCCLUDE_CHANNELS = 1, C3_OCCLUDE_BANDS = 2, or both = 3)", who, what);
    if (band < 1 || band > m->positions) return fail("%s: band %d outside 1 .. %d, the window's positions", who, band, m->positions);
    return 0;
}

// in_host: the staged units of the call back to back (full alignment: the occupied rows, with one checked first[] / count[] entry per
// window; pileup: the windows themselves, first = count = null)
static int occlude_run(c3_model *m, const char *who, const int8_t *in_host, int x_dtype, const int32_t *first, const int32_t *count, int64_t batch,
                       const OccludePlan &plan, float *y_host, c3_occlude_window *out, float *drops_out, float *variant_rows_out, c3_occlude_info *info) {
    const bool fa = m->kind == C3_KIND_FULL_ALIGNMENT;
    const size_t unit_bytes = fa ? (size_t)m->positions * m->C : (size_t)c3_model_window_bytes(m, x_dtype);
    const int K = plan.K();
    const std::vector<OccludePass> passes = occlude_cut(count, batch, occlude_chunk_env(m->kind), K);
    size_t need = 0;
    for (const OccludePass &ps : passes) {
        if (ps.dense() > INT32_MAX) return fail("%s: %lld dense windows in one pass: set C3HIP_OCCLUDE_CHUNK", who, (long long)ps.dense());
        need = std::max(need, OccludeLayout(ps, unit_bytes, m->row, drops_out != nullptr).bytes);
    }
    HIP_TRY(hipSetDevice(m->device));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    TRY(ensure_occlude_buf(m, need));
    // the forms the handle is on, for this call alone: what it reports, taps, profiles and counts stays as it is (jackknife_run does the same)
    const c3_model::Choices reported = m->choice;
    const bool f16 = m->f16_ok, tap_call = m->tap_call, prof = m->prof;
    const int64_t tap_base = m->tap_base;
    const uint32_t tap_mask = m->tap_mask;
    int rc = 0, on_fp32 = 0;
    size_t staged = 0;
    JackknifeTimer t_expand, t_reduce;
    t_expand.on = t_reduce.on = info != nullptr;
    std::vector<OccludeEntry> tab;
    char *base = (char *)m->occlude_dev;
    for (const OccludePass &ps : passes) {
        const OccludeLayout L(ps, unit_bytes, m->row, drops_out != nullptr);
        tab.assign((size_t)ps.dense(), OccludeEntry{});
        occlude_fill_pass(tab.data(), ps, plan, first, count, unit_bytes);
        if (ps.units) rc = h2d_staged(base + L.in_at, in_host + (size_t)ps.unit0 * unit_bytes, (size_t)ps.units * unit_bytes, s);
        if (rc == 0) rc = h2d_staged(base + L.tab_at, tab.data(), L.tab_bytes(), s);
        if (rc) break;
        staged += (size_t)ps.units * unit_bytes + L.tab_bytes();
        float *y = (float *)(base + L.y_at);
        OccludeReduceParams rp;
        rp.base = y, rp.variants = y + ps.windows * m->row, rp.out = (c3_occlude_window *)(base + L.rec_at);
        rp.drops = drops_out ? (float *)(base + L.drops_at) : nullptr, rp.stride = m->row, rp.nout = m->nout, rp.batch = (int)ps.windows;
        rp.channels = plan.channels, rp.bands = plan.bands;
        for (int attempt = 0; attempt < 2 && rc == 0; ++attempt) {
            // full alignment: the fp16x3 forms raise the range flag; the fp32 forms of the second attempt do not look at it.  A pileup handle
            // has no such guard
            const bool guarded = fa && f16 && attempt == 0;
            m->f16_ok = attempt == 0 ? f16 : false, m->tap_call = true, m->prof = false, m->tap_mask = 0;
            rc = occlude_forward(m, s, (const int8_t *)(base + L.in_at), (const OccludeEntry *)(base + L.tab_at), ps.dense(), x_dtype, y, t_expand);
            m->f16_ok = f16, m->tap_call = tap_call, m->prof = prof, m->tap_base = tap_base, m->tap_mask = tap_mask, m->choice = reported;
            if (rc) break;
            if (guarded) {  // a non-finite row raises bit 1 of the flag as in the ring
                const int64_t nf = ps.dense() * m->row;
                hipLaunchKernelGGL(rows_finite_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, y, nf, m->range_flag);
                if (hipGetLastError() != hipSuccess) {
                    rc = fail("%s: the scan of the rows could not be launched", who);
                    break;
                }
            }
            if ((rc = occlude_reduce_launch(s, rp, &t_reduce)) != 0) break;
            // the records and, behind them, the pass's copy of the range flag come home in one copy: the one place the host waits for the pass
            if (guarded && hipMemcpyAsync(base + L.flag_at, m->range_flag, 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
                rc = fail("%s: hipMemcpyAsync failed", who);
                break;
            }
            std::vector<char> home(L.flag_at + (guarded ? 4 : 0) - L.rec_at);
            if ((rc = d2h_staged(home.data(), base + L.rec_at, home.size(), s)) != 0) break;
            uint32_t flag = 0;
            if (guarded) memcpy(&flag, home.data() + home.size() - 4, 4);
            if (guarded && flag) {  // beyond the range of the fp16x3 kernels: this pass again on the fp32-MFMA forms, for this call alone
                if (hipMemsetAsync(m->range_flag, 0, 256, s) != hipSuccess) rc = fail("%s: hipMemsetAsync failed", who);
                on_fp32 = 1;
                continue;
            }
            memcpy(out + ps.w0, home.data(), (size_t)ps.windows * sizeof(c3_occlude_window));
            if (y_host) rc = d2h_staged(y_host + ps.w0 * m->row, y, (size_t)ps.windows * m->row * sizeof(float), s);
            if (rc == 0 && drops_out && ps.variants) rc = d2h_staged(drops_out + ps.var0 * 4, base + L.drops_at, (size_t)ps.variants * 4 * sizeof(float), s);
            if (rc == 0 && variant_rows_out && ps.variants)
                rc = d2h_staged(variant_rows_out + ps.var0 * m->row, y + ps.windows * m->row, (size_t)ps.variants * m->row * sizeof(float), s);
            break;
        }
        if (rc) break;
    }
    if (rc) {
        const std::string why = g_err;
        (void)hipStreamSynchronize(s);
        (void)t_expand.total_us(), (void)t_reduce.total_us();
        return g_err = why, rc;
    }
    const float expand_us = t_expand.total_us(), reduce_us = t_reduce.total_us();  // (the last copy home has synchronised the stream)
    if (info) {
        *info = c3_occlude_info{};
        info->expand_us = expand_us, info->reduce_us = reduce_us;
        info->windows = batch, info->variants = batch * K, info->passes = (int64_t)passes.size(), info->bytes_staged = (int64_t)staged, info->on_fp32 = on_fp32;
    }
    return 0;
}

extern "C" {

int c3_occlude_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, int what, int band,
                    float *y_host, c3_occlude_window *out, float *drops_out, float *variant_rows_out, c3_occlude_info *info) {
    TRY(occlude_handle(m, "c3_occlude_rows", what, band));
    if (m->kind != C3_KIND_FULL_ALIGNMENT) return fail("c3_occlude_rows: occupied rows are full-alignment input: a pileup handle takes its windows through c3_occlude");
    if (batch < 0) return fail("negative batch");
    if (batch > 0 && (!row_count || !out)) return fail("null buffer: row_count / out");
    std::vector<int32_t> first((size_t)batch), count((size_t)batch);
    int64_t total = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const int32_t c = table_i32(row_count, b);
        if (c < 0) return fail("window %lld: negative row_count %d", (long long)b, c);
        const int32_t f = row_first ? table_i32(row_first, b) : (m->depth - c) / 2;
        if (f < 0) return fail("window %lld: negative row_first %d", (long long)b, f);
        if ((int64_t)f + c > m->depth)
            return fail("window %lld: rows [%d, %lld) reach beyond the depth of %d rows", (long long)b, f, (long long)f + c, m->depth);
        first[(size_t)b] = f, count[(size_t)b] = c, total += c;
    }
    if (total > 0 && !rows_host) return fail("null buffer: rows");
    if (info) *info = c3_occlude_info{};
    if (batch == 0) return 0;
    return occlude_run(m, "c3_occlude_rows", (const int8_t *)rows_host, C3_DTYPE_I8, first.data(), count.data(), batch,
                       OccludePlan(m->positions, m->C, what, band), y_host, out, drops_out, variant_rows_out, info);
}

int c3_occlude(c3_model *m, const void *x_host, int x_dtype, int64_t batch, int what, int band, float *y_host, c3_occlude_window *out,
               float *drops_out, float *variant_rows_out, c3_occlude_info *info) {
    TRY(occlude_handle(m, "c3_occlude", what, band));
    if (batch < 0) return fail("negative batch");
    if (m->kind == C3_KIND_FULL_ALIGNMENT && x_dtype != C3_DTYPE_I8) return fail("full-alignment windows must be int8 (got dtype %d)", x_dtype);
    if (m->kind == C3_KIND_PILEUP && x_dtype != C3_DTYPE_I8 && x_dtype != C3_DTYPE_I32)
        return fail("pileup windows must be int8 or int32 (got dtype %d)", x_dtype);
    if (batch > 0 && (!x_host || !out)) return fail("null buffer: windows / out");
    if (info) *info = c3_occlude_info{};
    if (batch == 0) return 0;
    const OccludePlan plan(m->positions, m->C, what, band);
    if (m->kind == C3_KIND_PILEUP)
        return occlude_run(m, "c3_occlude", (const int8_t *)x_host, x_dtype, nullptr, nullptr, batch, plan, y_host, out, drops_out, variant_rows_out, info);
    // every window's run, found on the host as c3_pack_rows finds it; its first row is the run's own.  Only the occupied rows are staged
    const size_t row_bytes = (size_t)m->positions * m->C, wbytes = (size_t)m->depth * row_bytes;
    std::vector<int32_t> first((size_t)batch), count((size_t)batch);
    size_t total = 0;
    for (int64_t b = 0; b < batch; ++b) {
        occupied_run((const uint8_t *)x_host + (size_t)b * wbytes, m->depth, row_bytes, &first[(size_t)b], &count[(size_t)b]);
        total += (size_t)count[(size_t)b];
    }
    std::vector<int8_t> rows(std::max<size_t>(total * row_bytes, 1));
    size_t at = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const size_t n = (size_t)count[(size_t)b] * row_bytes;
        memcpy(rows.data() + at, (const char *)x_host + (size_t)b * wbytes + (size_t)first[(size_t)b] * row_bytes, n);
        at += n;
    }
    return occlude_run(m, "c3_occlude", rows.data(), C3_DTYPE_I8, first.data(), count.data(), batch, plan, y_host, out, drops_out, variant_rows_out, info);
}

int c3_occlude_reduce(c3_model *m, const float *base_rows, const float *variant_rows, int row_floats, int channels, int bands, int64_t batch,
                      c3_occlude_window *out, float *drops_out) {
    if (!m) return fail("null model");
    if (batch < 0) return fail("negative batch");
    if (batch > INT32_MAX) return fail("c3_occlude_reduce: too many windows for one call (%lld)", (long long)batch);
    if (channels < 0 || bands < 0 || (int64_t)channels + bands > INT32_MAX)
        return fail("c3_occlude_reduce: group sizes %d and %d: both must be >= 0 and add up to an int32", channels, bands);
    if (row_floats != m->nout && row_floats != m->nout + kDecodeCols)
        return fail("c3_occlude_reduce: rows of %d floats: this model has %d probabilities, %d with the decoder columns", row_floats, m->nout, m->nout + kDecodeCols);
    if (batch == 0) return 0;
    if (!base_rows || !out) return fail("null buffer: base_rows / out");
    const int64_t K = (int64_t)channels + bands, total = batch * K;
    if (total > 0 && !variant_rows) return fail("null buffer: variant_rows");
    HIP_TRY(hipSetDevice(m->device));
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t rf = (size_t)row_floats * sizeof(float);
    const size_t v_at = al((size_t)batch * rf), r_at = al(v_at + (size_t)total * rf), d_at = al(r_at + (size_t)batch * sizeof(c3_occlude_window));
    TRY(ensure_occlude_buf(m, d_at + (drops_out ? (size_t)total * 16 : 0)));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    char *base = (char *)m->occlude_dev;
    TRY(h2d_staged(base, base_rows, (size_t)batch * rf, s));
    if (total) TRY(h2d_staged(base + v_at, variant_rows, (size_t)total * rf, s));
    OccludeReduceParams rp;
    rp.base = (const float *)base, rp.variants = (const float *)(base + v_at), rp.out = (c3_occlude_window *)(base + r_at);
    rp.drops = drops_out ? (float *)(base + d_at) : nullptr, rp.stride = row_floats, rp.nout = m->nout, rp.batch = (int)batch;
    rp.channels = channels, rp.bands = bands;
    TRY(occlude_reduce_launch(s, rp));
    TRY(d2h_staged(out, base + r_at, (size_t)batch * sizeof(c3_occlude_window), s));
    if (drops_out && total) TRY(d2h_staged(drops_out, base + d_at, (size_t)total * 16, s));
    return 0;
}

}  // extern "C"
