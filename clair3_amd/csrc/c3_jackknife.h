// c3_jackknife.h -- jackknife mode (c3_jackknife_rows, c3_jackknife, c3_jackknife_reduce): what the INPUT does to a label.  For
// every full-alignment window of a call the device builds the row_count[b] leave-one-read-out variants from the window's staged rows
// (c3_expand.h stages them once), runs them through the unchanged forward pass beside the window itself and reduces their rows to one
// 80-byte record per window.  An instrument like the audit, not a path of a pipeline: nothing is allocated, launched or planned unless one of
// the three entries is called.  The rule in numpy: synthetic.leave_one_out / jackknife_records.
//
// THE definitions (include/c3hip.h, the numpy rule and the kernels below cite this block; tests/test_jackknife.py holds them together).
// Window b has n = row_count[b] reads -- the rows of its run, whatever they hold: an interior all-zero row of the run is a read too --,
// base row y and variants v_0 .. v_{n-1}, variant j being the window without row j of its run:
//   layout          C3_JACKKNIFE_RECENTRE (0): the n - 1 rows that stay start at dense row (depth - (n - 1)) / 2, the reference's padding rule
//                   (clair3/utils.py:113-121) applied to the variant's own count -- the window its producer would have laid out without that
//                   read.  C3_JACKKNIFE_IN_PLACE (1): they start at the base window's first row.  The base window itself sits where
//                   row_first / the centring rule puts it, as in c3_predict_rows.  n = 1: one variant, the all-zero window
//   arg-max         of a head: the first maximum by `>` from -inf on -- lowest index on ties, a NaN never, the head's first column when
//                   nothing exceeds -inf (the rule of c3_census.h and c3_refine.h).  Heads are columns (0,21) (21,24) (24,57) (57,90) limited
//                   to nout
//   nonfinite       variants with a probability among their first nout columns that is not finite
//   flips[h]        variants whose arg-max in head h differs from the base row's, non-finite variants included (0 for a head the model lacks)
//   decision_flips  rows with decoder columns (stride > nout; c3_decode.h): per reference base b of A C G T the variants whose decoder
//                   column 23 + b compares unequal (float !=) to the base row's; rows without decoder columns: 0
//   drop            of variant j in head h: y[t] - v_j[t] in one float32 subtraction, t the base row's arg-max of the head (0 for a head the
//                   model lacks)
//   lean_read[h]    the j with the largest drop among the variants that are finite and whose drop is not a NaN (a NaN base row has none),
//                   the lowest j on ties; -1 when there is no such variant.  lean_drop[h]: that drop (may be negative), 0 with lean_read -1
//   max_delta       max over the finite variants and the first nout columns of |v_j[c] - y[c]| in float32, differences that are NaN left
//                   out; 0 without any
//   n = 0           the all-zero record with lean_read = -1
// Only integer counts, comparisons and single float32 subtractions: the record is exactly what the numpy rule gives on the same rows.
//
// Launches (the active lane's stream; no atomics, nothing depends on scheduling):
//   jackknife_expand_kernel<V>   expand_rows_kernel (c3_expand.h) with one source row left out: one workgroup per dense window to build
//   jackknife_reduce_kernel      one wave per window, lanes striding over its variants; counts are summed and maxima taken by a butterfly on
//                                keys (value bits, then lowest index) as outcome_maxima_kernel does
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

namespace c3 {

#define C3_JACKKNIFE_TEXT __attribute__((section(".c3_jackknife_text")))  // behind `.c3_refine_text`: no other kernel moves

// one per dense window to build, filled by the host (jackknife_fill_pass)
struct JackknifeEntry {
    int64_t src;    // byte offset of the window's first occupied row in the pass's staged rows
    int32_t first;  // dense row the output run starts at
    int32_t count;  // source rows
    int32_t skip;   // >= 0: the source row to leave out; -1: the plain window
    int32_t pad;
};
static_assert(sizeof(JackknifeEntry) == 24, "JackknifeEntry is 24 bytes");

struct JackknifeExpandParams {
    const int8_t *rows;         // the pass's staged rows
    const JackknifeEntry *tab;  // [B]
    int8_t *out;                // [B][depth][positions * C] dense windows
    int B;
    int row_bytes, window_bytes;  // positions * C, depth * row_bytes
};

// One workgroup per dense window, the entry workgroup-uniform.  With rp = row_bytes / V pieces a row, lo = first * rp and
// hi = lo + (count - (skip >= 0)) * rp, destination piece p is zero outside [lo, hi) and source piece q = p - lo inside, moved on by one row
// (rp) from the left-out row on: no division, no per-row lookup, every destination byte written exactly once, no memset, no atomics.
// V = 8 / V = 1 as expand_rows_kernel: 8-byte pieces for an even channel count, bytes for the dwell model's 297-byte rows.
template <int V>
__global__ __launch_bounds__(kExpandThreads) C3_JACKKNIFE_TEXT void jackknife_expand_kernel(JackknifeExpandParams p) {
    const int b = blockIdx.x;
    if (b >= p.B) return;
    const JackknifeEntry e = p.tab[b];
    const int rp = p.row_bytes / V, n = p.window_bytes / V;
    const int lo = e.first * rp, hi = lo + (e.count - (e.skip >= 0 ? 1 : 0)) * rp;
    const int cut = e.skip >= 0 ? e.skip * rp : n;  // source pieces from here on belong to the row behind (q < n always: no cut)
    if constexpr (V == 8) {
        const uint2 *src = reinterpret_cast<const uint2 *>(p.rows + e.src);
        uint2 *dst = reinterpret_cast<uint2 *>(p.out + (int64_t)b * p.window_bytes);
        for (int i = threadIdx.x; i < n; i += kExpandThreads) {
            uint2 v = make_uint2(0u, 0u);
            if (i >= lo && i < hi) {
                const int q = i - lo;
                v = src[q >= cut ? q + rp : q];
            }
            dst[i] = v;
        }
    } else {
        const int8_t *src = p.rows + e.src;
        int8_t *dst = p.out + (int64_t)b * p.window_bytes;
        for (int i = threadIdx.x; i < n; i += kExpandThreads) {
            int8_t v = 0;
            if (i >= lo && i < hi) {
                const int q = i - lo;
                v = src[q >= cut ? q + rp : q];
            }
            dst[i] = v;
        }
    }
}

struct JackknifeReduceParams {
    const float *base;         // [batch][stride]: the windows' own rows
    const float *variants;     // [sum count][stride]: the variants' rows, window after window in read order
    const int64_t *var_first;  // [batch] the window's first variant
    const int32_t *count;      // [batch]
    c3_jackknife_window *out;  // [batch]
    float *drops;              // [sum count][4], or null
    int stride, nout, batch;
};

// float -> key whose unsigned order is the float order (negative drops occur; -0 takes the key of +0: the two are a tie), and back
__device__ __forceinline__ uint32_t jackknife_key(float x) {
    const uint32_t bits = __float_as_uint(x), u = bits == 0x80000000u ? 0u : bits;
    return u & 0x80000000u ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float jackknife_unkey(uint32_t k) { return __uint_as_float(k & 0x80000000u ? k & 0x7fffffffu : ~k); }

__global__ __launch_bounds__(64) C3_JACKKNIFE_TEXT void jackknife_reduce_kernel(JackknifeReduceParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= p.batch) return;
    const float *y = p.base + (int64_t)b * p.stride;
    const int n = p.count[b];
    const int64_t at = p.var_first[b];
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
    uint32_t nonfinite = 0, flips[4] = {0, 0, 0, 0}, dflips[4] = {0, 0, 0, 0}, delta = 0;  // delta: bits of a float >= 0
    unsigned long long lean[4] = {0, 0, 0, 0};  // key of the drop << 32 | ~j; 0: none
    for (int j = lane; j < n; j += 64) {
        const float *v = p.variants + (at + j) * p.stride;
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
            flips[h] += am[h] != t[h];
            if (finite && drop == drop) {
                const unsigned long long key = (unsigned long long)jackknife_key(drop) << 32 | (uint32_t)~(uint32_t)j;
                lean[h] = key > lean[h] ? key : lean[h];
            }
        }
        if (cols) {
#pragma unroll
            for (int k = 0; k < 4; ++k) dflips[k] += v[p.nout + 23 + k] != y[p.nout + 23 + k];
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        nonfinite += __shfl_xor(nonfinite, off, 64);
        delta = max(delta, (uint32_t)__shfl_xor(delta, off, 64));
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            flips[h] += __shfl_xor(flips[h], off, 64), dflips[h] += __shfl_xor(dflips[h], off, 64);
            const unsigned long long o = __shfl_xor(lean[h], off, 64);
            lean[h] = o > lean[h] ? o : lean[h];
        }
    }
    if (lane != 0) return;
    c3_jackknife_window r;
    r.reads = n, r.nonfinite = (int32_t)nonfinite;
    for (int h = 0; h < 4; ++h) {
        r.flips[h] = (int32_t)flips[h], r.decision_flips[h] = (int32_t)dflips[h];
        r.lean_read[h] = lean[h] ? (int32_t)~(uint32_t)lean[h] : -1;
        r.lean_drop[h] = lean[h] ? jackknife_unkey((uint32_t)(lean[h] >> 32)) : 0.f;
    }
    r.max_delta = __uint_as_float(delta), r.reserved = 0;
    p.out[b] = r;
}

// ------------------------------------------------------------------------------------------ the host's plan (plain host code: tests/host/
// jackknife_host_check.cpp drives it against buffers of exactly these sizes).  The pass, its cut and its layout are c3_variants.h's; one
// variant per read
static inline int64_t jackknife_chunk_env() { return variant_chunk_env("C3HIP_JACKKNIFE_CHUNK", 64); }  // windows per pass, 0 = never cut
static inline std::vector<VariantPass> jackknife_cut(const int32_t *count, int64_t batch, int64_t chunk) {
    return variant_cut(count, batch, chunk, [count](int64_t w) { return (int64_t)count[w]; });
}
// meta block: table | var_first | count (RunMeta); home: the 80-byte records; extra: the drops
static inline VariantLayout jackknife_layout(const VariantPass &ps, size_t row_bytes, int row_floats, bool drops) {
    return VariantLayout(ps, row_bytes, RunMeta(ps, sizeof(JackknifeEntry)).bytes, row_floats, (size_t)ps.windows * sizeof(c3_jackknife_window),
                         drops ? (size_t)ps.variants * 4 * sizeof(float) : 0);
}
// the meta block of a pass as it is staged, into `meta` of RunMeta(..).bytes bytes: the table (base entries with skip = -1 first, then every
// window's variants in window order, read order), every window's first variant (within the pass) and its count.  first[] / count[] are the
// call's, checked by the entry
static inline void jackknife_fill_pass(char *meta, const VariantPass &ps, const int32_t *first, const int32_t *count, int depth, size_t row_bytes,
                                       int layout) {
    const RunMeta M(ps, sizeof(JackknifeEntry));
    memset(meta, 0, M.bytes);  // (the gaps between the sections and the entries' padding)
    JackknifeEntry *tab = reinterpret_cast<JackknifeEntry *>(meta);
    int64_t *var_first = reinterpret_cast<int64_t *>(meta + M.var_first_at);
    int32_t *cnt = reinterpret_cast<int32_t *>(meta + M.count_at);
    int64_t row = 0, var = 0;
    for (int64_t i = 0; i < ps.windows; ++i) {
        const int32_t n = count[ps.w0 + i], f = first[ps.w0 + i];
        tab[i] = JackknifeEntry{(int64_t)(row * (int64_t)row_bytes), f, n, -1, 0};
        var_first[i] = var, cnt[i] = n;
        for (int32_t j = 0; j < n; ++j)
            tab[ps.windows + var + j] = JackknifeEntry{(int64_t)(row * (int64_t)row_bytes), layout == C3_JACKKNIFE_IN_PLACE ? f : (depth - (n - 1)) / 2, n, j, 0};
        row += n, var += n;
    }
}

}  // namespace c3

// ------------------------------------------------------------------------------------------ the entries (include/c3hip.h)
// the mode of variant_run (c3_variants.h).  first[] / count[]: one checked entry per window (first: the base window's)
struct JackknifeMode {
    static constexpr const char *chunk_var = "C3HIP_JACKKNIFE_CHUNK";
    c3_model *m;
    const int32_t *first, *count;
    int where;  // C3_JACKKNIFE_RECENTRE / _IN_PLACE
    c3_jackknife_window *out;
    float *drops_out;
    size_t row_bytes() const { return (size_t)m->positions * m->C; }
    VariantLayout layout(const VariantPass &ps) const { return jackknife_layout(ps, row_bytes(), m->row, drops_out != nullptr); }
    void fill(char *meta, const VariantPass &ps) const { jackknife_fill_pass(meta, ps, first, count, m->depth, row_bytes(), where); }
    int expand(hipStream_t s, VariantTimer &timer, const int8_t *rows, const char *meta, char *, int64_t off, int64_t n, void *dst) const {
        const JackknifeExpandParams ep{rows, (const JackknifeEntry *)meta + off, (int8_t *)dst, (int)n, m->positions * m->C,
                                       (int)c3_model_window_bytes(m, C3_DTYPE_I8)};
        if (ep.row_bytes % 8 == 0) return variant_launch(s, &timer, jackknife_expand_kernel<8>, n, kExpandThreads, ep);
        return variant_launch(s, &timer, jackknife_expand_kernel<1>, n, kExpandThreads, ep);
    }
    int reduce(hipStream_t s, VariantTimer &timer, const VariantPass &ps, const VariantLayout &L, char *base) const {
        const RunMeta M(ps, sizeof(JackknifeEntry));
        float *y = (float *)(base + L.y_at);
        JackknifeReduceParams rp;
        rp.base = y, rp.variants = y + ps.windows * m->row, rp.var_first = (const int64_t *)(base + L.meta_at + M.var_first_at);
        rp.count = (const int32_t *)(base + L.meta_at + M.count_at), rp.out = (c3_jackknife_window *)(base + L.home_at);
        rp.drops = drops_out ? (float *)(base + L.extra_at) : nullptr, rp.stride = m->row, rp.nout = m->nout, rp.batch = (int)ps.windows;
        return variant_launch(s, &timer, jackknife_reduce_kernel, rp.batch, 64, rp);
    }
    int deliver(hipStream_t s, const VariantPass &ps, const char *home, const char *drops) const {
        memcpy(out + ps.w0, home, (size_t)ps.windows * sizeof(c3_jackknife_window));
        return drops_out && ps.variants ? d2h_staged(drops_out + ps.var0 * 4, drops, (size_t)ps.variants * 4 * sizeof(float), s) : 0;
    }
};

// what the two entries that run the network tell a pileup handle
static const char kJackknifeFaOnly[] =
    "%s: the jackknife leaves out reads of full-alignment windows: a pileup window holds counts, not reads (c3_jackknife_reduce serves its rows)";

extern "C" {

int c3_jackknife_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, int layout,
                      float *y_host, c3_jackknife_window *out, float *drops_out, float *variant_rows_out, c3_jackknife_info *info) {
    TRY(variant_handle(m, "c3_jackknife_rows", kJackknifeFaOnly));
    if (batch < 0) return fail("negative batch");
    if (layout != C3_JACKKNIFE_RECENTRE && layout != C3_JACKKNIFE_IN_PLACE)
        return fail("c3_jackknife_rows: unknown layout %d (C3_JACKKNIFE_RECENTRE or C3_JACKKNIFE_IN_PLACE)", layout);
    if (batch > 0 && (!row_count || !out)) return fail("null buffer: row_count / out");
    std::vector<int32_t> first, count;
    int64_t total = 0;
    TRY(checked_runs(m, row_first, row_count, batch, &first, &count, &total));
    if (total > 0 && !rows_host) return fail("null buffer: rows");
    if (info) *info = c3_jackknife_info{};
    if (batch == 0) return 0;
    const JackknifeMode mode{m, first.data(), count.data(), layout, out, drops_out};
    return variant_run(m, "c3_jackknife_rows", (const int8_t *)rows_host, C3_DTYPE_I8, jackknife_cut(count.data(), batch, jackknife_chunk_env()), mode,
                       y_host, variant_rows_out, info);
}

int c3_jackknife(c3_model *m, const void *x_host, int x_dtype, int64_t batch, int layout, float *y_host, c3_jackknife_window *out,
                 float *drops_out, float *variant_rows_out, c3_jackknife_info *info) {
    TRY(variant_handle(m, "c3_jackknife", kJackknifeFaOnly));
    if (batch < 0) return fail("negative batch");
    if (x_dtype != C3_DTYPE_I8) return fail("full-alignment windows must be int8 (got dtype %d)", x_dtype);
    if (layout != C3_JACKKNIFE_RECENTRE && layout != C3_JACKKNIFE_IN_PLACE)
        return fail("c3_jackknife: unknown layout %d (C3_JACKKNIFE_RECENTRE or C3_JACKKNIFE_IN_PLACE)", layout);
    if (batch > 0 && (!x_host || !out)) return fail("null buffer: windows / out");
    if (info) *info = c3_jackknife_info{};
    if (batch == 0) return 0;
    std::vector<int32_t> first, count;
    std::vector<int8_t> rows;
    gather_runs(m, x_host, batch, &first, &count, &rows);
    const JackknifeMode mode{m, first.data(), count.data(), layout, out, drops_out};
    return variant_run(m, "c3_jackknife", rows.data(), C3_DTYPE_I8, jackknife_cut(count.data(), batch, jackknife_chunk_env()), mode, y_host,
                       variant_rows_out, info);
}

int c3_jackknife_reduce(c3_model *m, const float *base_rows, const float *variant_rows, int row_floats, const int32_t *row_count, int64_t batch,
                        c3_jackknife_window *out, float *drops_out) {
    if (!m) return fail("null model");
    if (batch < 0) return fail("negative batch");
    if (batch > INT32_MAX) return fail("c3_jackknife_reduce: too many windows for one call (%lld)", (long long)batch);
    if (row_floats != m->nout && row_floats != m->nout + kDecodeCols)
        return fail("c3_jackknife_reduce: rows of %d floats: this model has %d probabilities, %d with the decoder columns", row_floats, m->nout, m->nout + kDecodeCols);
    if (batch == 0) return 0;
    if (!base_rows || !row_count || !out) return fail("null buffer: base_rows / row_count / out");
    std::vector<int64_t> var_first((size_t)batch);
    std::vector<int32_t> count((size_t)batch);
    int64_t total = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const int32_t c = table_i32(row_count, b);
        if (c < 0) return fail("window %lld: negative row_count %d", (long long)b, c);
        var_first[(size_t)b] = total, count[(size_t)b] = c, total += c;
    }
    if (total > 0 && !variant_rows) return fail("null buffer: variant_rows");
    HIP_TRY(hipSetDevice(m->device));
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t rf = (size_t)row_floats * sizeof(float);
    const size_t v_at = al((size_t)batch * rf), f_at = al(v_at + (size_t)total * rf), c_at = al(f_at + (size_t)batch * 8), r_at = al(c_at + (size_t)batch * 4);
    const size_t d_at = al(r_at + (size_t)batch * sizeof(c3_jackknife_window));
    TRY(ensure_variant_buf(m, d_at + (drops_out ? (size_t)total * 16 : 0)));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    char *base = (char *)m->variant_dev;
    TRY(h2d_staged(base, base_rows, (size_t)batch * rf, s));
    if (total) TRY(h2d_staged(base + v_at, variant_rows, (size_t)total * rf, s));
    TRY(h2d_staged(base + f_at, var_first.data(), (size_t)batch * 8, s));
    TRY(h2d_staged(base + c_at, count.data(), (size_t)batch * 4, s));
    JackknifeReduceParams rp;
    rp.base = (const float *)base, rp.variants = (const float *)(base + v_at), rp.var_first = (const int64_t *)(base + f_at);
    rp.count = (const int32_t *)(base + c_at), rp.out = (c3_jackknife_window *)(base + r_at), rp.drops = drops_out ? (float *)(base + d_at) : nullptr;
    rp.stride = row_floats, rp.nout = m->nout, rp.batch = (int)batch;
    TRY(variant_launch(s, nullptr, jackknife_reduce_kernel, batch, 64, rp));
    TRY(d2h_staged(out, base + r_at, (size_t)batch * sizeof(c3_jackknife_window), s));
    if (drops_out && total) TRY(d2h_staged(drops_out, base + d_at, (size_t)total * 16, s));
    return 0;
}

}  // extern "C"
