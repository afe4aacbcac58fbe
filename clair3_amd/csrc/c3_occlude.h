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
// The pass, its cut and its layout are c3_variants.h's.  env C3HIP_OCCLUDE_CHUNK: windows per pass, 0 = never cut; default 64
// full-alignment windows (jackknife mode's pass), 256 pileup windows (256 * 52 dense windows stay below the pileup micro-batch of 16384)
static inline int64_t occlude_chunk_env(int kind) { return variant_chunk_env("C3HIP_OCCLUDE_CHUNK", kind == C3_KIND_PILEUP ? 256 : 64); }
// count: the windows' occupied rows (full alignment), or null: one unit a window (pileup); K variants a window
static inline std::vector<VariantPass> occlude_cut(const int32_t *count, int64_t batch, int64_t chunk, int K) {
    return variant_cut(count, batch, chunk, [K](int64_t) { return (int64_t)K; });
}
// meta block: the table alone; home: the 144-byte records; extra: the drops
static inline VariantLayout occlude_layout(const VariantPass &ps, size_t unit_bytes, int row_floats, bool drops) {
    return VariantLayout(ps, unit_bytes, (size_t)ps.dense() * sizeof(OccludeEntry), row_floats, (size_t)ps.windows * sizeof(c3_occlude_window),
                         drops ? (size_t)ps.variants * 4 * sizeof(float) : 0);
}
// the table of a pass as it is staged, `tab` of ps.dense() entries: the base entries first (no mask), then every window's K variants in
// window order and variant order -- channels 0 .. C - 1, then bands 0 .. nb - 1.  first[] / count[] are the call's, checked by the entry
// (full alignment), or null (pileup: one unit of unit_bytes a window)
static inline void occlude_fill_pass(OccludeEntry *tab, const VariantPass &ps, const OccludePlan &plan, const int32_t *first, const int32_t *count,
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
// the mode of variant_run (c3_variants.h).  Full alignment: one checked first[] / count[] entry per window; pileup: the windows themselves
// are the staged units, first = count = null
struct OccludeMode {
    static constexpr const char *chunk_var = "C3HIP_OCCLUDE_CHUNK";
    c3_model *m;
    int x_dtype;
    const int32_t *first, *count;
    OccludePlan plan;
    c3_occlude_window *out;
    float *drops_out;
    size_t unit_bytes() const { return m->kind == C3_KIND_FULL_ALIGNMENT ? (size_t)m->positions * m->C : (size_t)c3_model_window_bytes(m, x_dtype); }
    VariantLayout layout(const VariantPass &ps) const { return occlude_layout(ps, unit_bytes(), m->row, drops_out != nullptr); }
    void fill(char *meta, const VariantPass &ps) const { occlude_fill_pass((OccludeEntry *)meta, ps, plan, first, count, unit_bytes()); }
    int expand(hipStream_t s, VariantTimer &timer, const int8_t *in, const char *meta, char *, int64_t off, int64_t n, void *dst) const {
        const bool fa = m->kind == C3_KIND_FULL_ALIGNMENT;
        const OccludeExpandParams ep{in, (const OccludeEntry *)meta + off, dst, (int)n, m->positions, m->C, m->positions * m->C,
                                     (int)c3_model_window_bytes(m, x_dtype)};
        if (fa && m->C == 8) return variant_launch(s, &timer, occlude_expand_kernel<8>, n, kExpandThreads, ep);  // (a piece is a cell only when C == 8)
        if (fa) return variant_launch(s, &timer, occlude_expand_kernel<1>, n, kExpandThreads, ep);
        if (x_dtype == C3_DTYPE_I8) return variant_launch(s, &timer, occlude_pileup_expand_kernel<int8_t>, n, kExpandThreads, ep);
        return variant_launch(s, &timer, occlude_pileup_expand_kernel<int32_t>, n, kExpandThreads, ep);
    }
    int reduce(hipStream_t s, VariantTimer &timer, const VariantPass &ps, const VariantLayout &L, char *base) const {
        float *y = (float *)(base + L.y_at);
        OccludeReduceParams rp;
        rp.base = y, rp.variants = y + ps.windows * m->row, rp.out = (c3_occlude_window *)(base + L.home_at);
        rp.drops = drops_out ? (float *)(base + L.extra_at) : nullptr, rp.stride = m->row, rp.nout = m->nout, rp.batch = (int)ps.windows;
        rp.channels = plan.channels, rp.bands = plan.bands;
        return variant_launch(s, &timer, occlude_reduce_kernel, rp.batch, 64, rp);
    }
    int deliver(hipStream_t s, const VariantPass &ps, const char *home, const char *drops) const {
        memcpy(out + ps.w0, home, (size_t)ps.windows * sizeof(c3_occlude_window));
        return drops_out && ps.variants ? d2h_staged(drops_out + ps.var0 * 4, drops, (size_t)ps.variants * 4 * sizeof(float), s) : 0;
    }
};

// what the two entries that run the network refuse before anything is queued
static int occlude_handle(c3_model *m, const char *who, int what, int band) {
    TRY(variant_handle(m, who, nullptr));
    if (what < 1 || what > 3) return fail("%s: unknown `what` %d (C3_OCCLUDE_CHANNELS = 1, C3_OCCLUDE_BANDS = 2, or both = 3)", who, what);
    if (band < 1 || band > m->positions) return fail("%s: band %d outside 1 .. %d, the window's positions", who, band, m->positions);
    return 0;
}

extern "C" {

int c3_occlude_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, int what, int band,
                    float *y_host, c3_occlude_window *out, float *drops_out, float *variant_rows_out, c3_occlude_info *info) {
    TRY(occlude_handle(m, "c3_occlude_rows", what, band));
    if (m->kind != C3_KIND_FULL_ALIGNMENT) return fail("c3_occlude_rows: occupied rows are full-alignment input: a pileup handle takes its windows through c3_occlude");
    if (batch < 0) return fail("negative batch");
    if (batch > 0 && (!row_count || !out)) return fail("null buffer: row_count / out");
    std::vector<int32_t> first, count;
    int64_t total = 0;
    TRY(checked_runs(m, row_first, row_count, batch, &first, &count, &total));
    if (total > 0 && !rows_host) return fail("null buffer: rows");
    if (info) *info = c3_occlude_info{};
    if (batch == 0) return 0;
    const OccludeMode mode{m, C3_DTYPE_I8, first.data(), count.data(), OccludePlan(m->positions, m->C, what, band), out, drops_out};
    return variant_run(m, "c3_occlude_rows", (const int8_t *)rows_host, C3_DTYPE_I8,
                       occlude_cut(count.data(), batch, occlude_chunk_env(m->kind), mode.plan.K()), mode, y_host, variant_rows_out, info);
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
    std::vector<int32_t> first, count;
    std::vector<int8_t> rows;
    const bool fa = m->kind == C3_KIND_FULL_ALIGNMENT;
    if (fa) gather_runs(m, x_host, batch, &first, &count, &rows);
    const OccludeMode mode{m, x_dtype, fa ? first.data() : nullptr, fa ? count.data() : nullptr, OccludePlan(m->positions, m->C, what, band), out, drops_out};
    return variant_run(m, "c3_occlude", fa ? rows.data() : (const int8_t *)x_host, x_dtype, occlude_cut(mode.count, batch, occlude_chunk_env(m->kind), mode.plan.K()),
                       mode, y_host, variant_rows_out, info);
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
    TRY(ensure_variant_buf(m, d_at + (drops_out ? (size_t)total * 16 : 0)));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    char *base = (char *)m->variant_dev;
    TRY(h2d_staged(base, base_rows, (size_t)batch * rf, s));
    if (total) TRY(h2d_staged(base + v_at, variant_rows, (size_t)total * rf, s));
    OccludeReduceParams rp;
    rp.base = (const float *)base, rp.variants = (const float *)(base + v_at), rp.out = (c3_occlude_window *)(base + r_at);
    rp.drops = drops_out ? (float *)(base + d_at) : nullptr, rp.stride = row_floats, rp.nout = m->nout, rp.batch = (int)batch;
    rp.channels = channels, rp.bands = bands;
    TRY(variant_launch(s, nullptr, occlude_reduce_kernel, batch, 64, rp));
    TRY(d2h_staged(out, base + r_at, (size_t)batch * sizeof(c3_occlude_window), s));
    if (drops_out && total) TRY(d2h_staged(drops_out, base + d_at, (size_t)total * 16, s));
    return 0;
}

}  // extern "C"
