// c3_subsample.h -- subsample mode (c3_subsample_rows, c3_subsample, c3_subsample_reduce): at what coverage does a call hold?
// The depth-titration counterpart of jackknife mode (c3_jackknife.h): for every full-alignment window of a call the device builds, for each
// of up to eight target depths, R random subsets of the window's reads from the rows staged once (c3_expand.h), runs them through the
// unchanged forward pass beside the window itself and reduces their rows to one 48-byte record per (window, level) and one 32-byte record
// per window.  The subsets are decided ON THE DEVICE from a stateless counter hash.  An instrument, not a path of a pipeline: nothing is
// allocated, launched or planned unless one of the three entries is called.  The rule in numpy: synthetic.subsample_keys / subsample_masks /
// subsample_variants / subsample_records.
//
// THE rule (include/c3hip.h, the numpy rule and the kernels below cite this block; tests/test_subsample.py holds them together).
// Window w -- its index in the CALL, not in a pass -- has n = row_count[w] reads: every row of its run is a read, an interior all-zero row of
// the run is a read too.  The call names `levels` target depths D_0 < D_1 < .. < D_{L-1} (1 <= L <= 8, every D >= 1), `replicates` R
// (1 <= R <= 32) and a uint64_t seed.
//   keys            key(w, r, j) = mix(seed + 0x9E3779B97F4A7C15 * (1 + (w * R + r) * depth + j)) of read j in replicate r, arithmetic mod
//                   2^64, depth the handle's, mix the SplitMix64 finaliser:
//                       z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
//                   The key does not depend on the level: a replicate's subsets are NESTED, its subset at D_l holds its subset at every
//                   smaller level
//   selection       at level l, k = min(n, D_l).  k == n: the level is NOT RUN for that window (its variant would be the window itself: it
//                   holds by definition).  k < n: R variants are run, replicate r keeping the k reads of smallest (key, j) -- rank by key,
//                   lowest j first on equal keys --; the kept reads stay in read order.  Always without replacement
//   layout          the two of jackknife mode with the same constants: C3_JACKKNIFE_RECENTRE (0): the kept rows start at dense row
//                   (depth - k) / 2, the reference's padding rule applied to the variant's own count.  C3_JACKKNIFE_IN_PLACE (1): they start at
//                   the base window's first row
//   order           of the variants: window by window, level by level (only levels that ran), replicate by replicate
//   arg-max         of a head and the head columns: c3_jackknife.h's -- the first maximum by `>` from -inf on, lowest index on ties, a NaN
//                   never, the head's first column when nothing exceeds -inf; columns (0,21) (21,24) (24,57) (57,90) limited to nout
// Per (window, level), c3_subsample_level (48 bytes), y the base row and t_h its arg-max in head h:
//   keep            k;  run: R or 0
//   nonfinite       variants with a probability among their first nout columns that is not finite
//   decision_flips  variants in which any of the decoder columns nout + 23 .. nout + 26 compares != to the base row's; rows without decoder
//                   columns (stride == nout): 0
//   flips[h]        variants whose arg-max in head h differs from t_h, non-finite variants included; 0 for a head the model lacks
//   min_kept[h]     the minimum over the level's finite variants of v[t_h]: the comparison is `<`, a NaN never wins, of equal values (-0 and
//                   +0) the lowest replicate's bits stay; when no finite variant ran the bits of the base row's own y[t_h]; 0 for a head the
//                   model lacks
// Per window, c3_subsample_window (32 bytes):
//   reads n, levels_run;  hold_level[h]: the lowest level index l such that flips[h] == 0 at l and at every deeper level -- levels that did
//   not run hold --, L when the deepest level itself flips, 0 for a head the model lacks;  hold_decision: the same over decision_flips;
//   reserved = 0.  n = 0: reads = 0, nothing run, every hold 0.
// Only integer counts, comparisons and copied float bits, no sums of floats: a record equals the numpy rule bit for bit on the same rows.
//
// Launches (the active lane's stream; no atomics, nothing depends on scheduling, every destination byte written exactly once, no memset):
//   subsample_expand_kernel<V>   one workgroup per dense window to build: keys into LDS, an O(n^2) rank, the kept reads compacted in read
//                                order, then the copy (V = 8 / 1 as expand_rows_kernel)
//   subsample_reduce_kernel      one wave per window, level by level, lanes striding over the level's replicates; counts are summed and
//                                minima taken by a butterfly as jackknife_reduce_kernel does
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

namespace c3 {

#define C3_SUBSAMPLE_TEXT __attribute__((section(".c3_subsample_text")))  // behind `.c3_jackknife_text`: no other kernel moves

constexpr int kSubsampleMaxDepth = 128;  // reads a workgroup ranks (the reference's depths are 89 and 55); deeper handles are refused
constexpr int kSubsampleMaxLevels = 8, kSubsampleMaxReplicates = 32;

// the counter hash of the rule (host and device: the host check rebuilds the device's selection with it)
__host__ __device__ inline uint64_t subsample_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__host__ __device__ inline uint64_t subsample_key(uint64_t seed, uint64_t w, uint64_t r, uint64_t j, uint64_t R, uint64_t depth) {
    return subsample_mix(seed + 0x9E3779B97F4A7C15ull * (1 + (w * R + r) * depth + j));
}

// one per dense window to build, filled by the host (subsample_fill_pass)
struct SubsampleEntry {
    int64_t src;        // byte offset of the window's first occupied row in the pass's staged rows
    int64_t window;     // the window's index in the CALL: the hash does not see the cut into passes
    int32_t first;      // dense row the output run starts at
    int32_t count;      // source rows: the window's reads
    int32_t keep;       // reads to keep; keep == count: the plain window
    int32_t replicate;  // r of the rule (0 for the plain window)
};
static_assert(sizeof(SubsampleEntry) == 32, "SubsampleEntry is 32 bytes");

struct SubsampleExpandParams {
    const int8_t *rows;         // the pass's staged rows
    const SubsampleEntry *tab;  // [B]
    int8_t *out;                // [B][depth][positions * C] dense windows
    uint64_t *masks;            // [B][2] kept-read bitmasks (bit j = read j kept), or null
    uint64_t seed;
    int B;
    int row_bytes, window_bytes;  // positions * C, depth * row_bytes
    int depth, replicates;        // of the rule's counter
};

// One workgroup per dense window, the entry workgroup-uniform.  Threads j < count hash their read's key into LDS; each then counts the reads
// whose (key, j) is smaller -- its rank; every lane reads the same LDS word at a time, a broadcast -- and is kept when rank < keep; its
// destination slot is the number of kept reads in front of it, and slot[] names the source row of every kept slot.  The copy then walks the
// window's pieces with (dense row, piece in row) carried along, no division in the loop: zero outside rows [first, first + keep), source row
// slot[row - first] inside.  count <= depth <= 128 (the entries check) bounds every LDS index, slot[] < count every source row.
template <int V>
__global__ __launch_bounds__(kExpandThreads) C3_SUBSAMPLE_TEXT void subsample_expand_kernel(SubsampleExpandParams p) {
    __shared__ uint64_t keys[kSubsampleMaxDepth];
    __shared__ uint8_t kept[kSubsampleMaxDepth], slot[kSubsampleMaxDepth];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= p.B) return;
    const SubsampleEntry e = p.tab[b];
    const int count = min(e.count, kSubsampleMaxDepth), keep = min(e.keep, count);
    const bool plain = keep >= count;
    if (!plain && tid < count) keys[tid] = subsample_key(p.seed, (uint64_t)e.window, (uint64_t)e.replicate, (uint64_t)tid, (uint64_t)p.replicates, (uint64_t)p.depth);
    __syncthreads();
    bool mine = false;
    if (tid < count) {
        mine = true;
        if (!plain) {
            const uint64_t k = keys[tid];
            int rank = 0;
            for (int i = 0; i < count; ++i) {
                const uint64_t o = keys[i];
                rank += o < k || (o == k && i < tid);
            }
            mine = rank < keep;
        }
        kept[tid] = mine;
    }
    __syncthreads();
    if (tid < count && mine) {
        int at = 0;
        for (int i = 0; i < tid; ++i) at += kept[i];
        slot[at] = (uint8_t)tid;
    }
    if (p.masks && tid < 128) {  // the first two waves, whole: read j is lane j of wave j / 64
        const unsigned long long bits = __ballot(mine);
        if ((tid & 63) == 0) p.masks[(int64_t)b * 2 + (tid >> 6)] = bits;
    }
    __syncthreads();
    const int rp = p.row_bytes / V, n = p.window_bytes / V;
    const int step_rows = kExpandThreads / rp, step_off = kExpandThreads % rp;
    int row = tid / rp, off = tid % rp;
    const int lo = e.first, hi = e.first + keep;
    if constexpr (V == 8) {
        const uint2 *src = reinterpret_cast<const uint2 *>(p.rows + e.src);
        uint2 *dst = reinterpret_cast<uint2 *>(p.out + (int64_t)b * p.window_bytes);
        for (int i = tid; i < n; i += kExpandThreads) {
            uint2 v = make_uint2(0u, 0u);
            if (row >= lo && row < hi) v = src[(int)slot[row - lo] * rp + off];
            dst[i] = v;
            row += step_rows, off += step_off;
            if (off >= rp) off -= rp, ++row;
        }
    } else {
        const int8_t *src = p.rows + e.src;
        int8_t *dst = p.out + (int64_t)b * p.window_bytes;
        for (int i = tid; i < n; i += kExpandThreads) {
            int8_t v = 0;
            if (row >= lo && row < hi) v = src[(int)slot[row - lo] * rp + off];
            dst[i] = v;
            row += step_rows, off += step_off;
            if (off >= rp) off -= rp, ++row;
        }
    }
}

struct SubsampleReduceParams {
    const float *base;           // [batch][stride]: the windows' own rows
    const float *variants;       // [variants][stride]: the variants' rows in the rule's order
    const int64_t *var_first;    // [batch] the window's first variant
    const int32_t *count;        // [batch] reads
    c3_subsample_level *levels;  // [batch][L]
    c3_subsample_window *out;    // [batch]
    int32_t depths[kSubsampleMaxLevels];
    int L, R;
    int stride, nout, batch;
};

__global__ __launch_bounds__(64) C3_SUBSAMPLE_TEXT void subsample_reduce_kernel(SubsampleReduceParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= p.batch) return;
    const float *y = p.base + (int64_t)b * p.stride;
    const int n = p.count[b];
    int64_t at = p.var_first[b];
    const bool cols = p.stride > p.nout;
    // the base row's arg-maxima (every lane: the loads are wave-uniform)
    int t[4], lo[4], hi[4];
    uint32_t yt[4];  // bits of y[t_h]
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        lo[h] = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
        hi[h] = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
        t[h] = lo[h], yt[h] = 0u;
        if (lo[h] >= hi[h]) continue;
        float best = -INFINITY;
        for (int c = lo[h]; c < hi[h]; ++c)
            if (y[c] > best) best = y[c], t[h] = c;
        yt[h] = __float_as_uint(y[t[h]]);
    }
    int hold[4] = {0, 0, 0, 0}, hold_decision = 0, levels_run = 0;
    for (int l = 0; l < p.L; ++l) {
        const int k = min(n, p.depths[l]);
        const bool run = k < n;
        uint32_t nonfinite = 0, dflips = 0, flips[4] = {0, 0, 0, 0};
        uint32_t mv[4] = {0, 0, 0, 0};                          // bits of the smallest v[t_h] of this lane's finite variants ...
        int mr[4] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};  // ... and its replicate; INT32_MAX: none
        if (run) {
            for (int r = lane; r < p.R; r += 64) {
                const float *v = p.variants + (at + r) * p.stride;
                bool finite = true;
                int am[4];
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    am[h] = lo[h];
                    float best = -INFINITY;
                    for (int c = lo[h]; c < hi[h]; ++c) {
                        const float x = v[c];
                        finite &= (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
                        if (x > best) best = x, am[h] = c;
                    }
                }
                nonfinite += !finite;
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    if (lo[h] >= hi[h]) continue;
                    flips[h] += am[h] != t[h];
                    const float x = v[t[h]];
                    if (finite && (mr[h] == INT32_MAX || x < __uint_as_float(mv[h]))) mv[h] = __float_as_uint(x), mr[h] = r;
                }
                if (cols) {
                    bool d = false;
#pragma unroll
                    for (int q = 0; q < 4; ++q) d |= v[p.nout + 23 + q] != y[p.nout + 23 + q];
                    dflips += d;
                }
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                nonfinite += __shfl_xor(nonfinite, off, 64), dflips += __shfl_xor(dflips, off, 64);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    flips[h] += __shfl_xor(flips[h], off, 64);
                    const uint32_t ov = __shfl_xor(mv[h], off, 64);
                    const int orr = __shfl_xor(mr[h], off, 64);
                    const float a = __uint_as_float(ov), m = __uint_as_float(mv[h]);
                    // the smaller value, of equal values the lower replicate: what a scan in replicate order with `<` keeps
                    if (orr != INT32_MAX && (mr[h] == INT32_MAX || a < m || (a == m && orr < mr[h]))) mv[h] = ov, mr[h] = orr;
                }
            }
            at += p.R, ++levels_run;
        }
        if (dflips) hold_decision = l + 1;
        c3_subsample_level rec;
        rec.keep = k, rec.run = run ? p.R : 0, rec.nonfinite = (int32_t)nonfinite, rec.decision_flips = (int32_t)dflips;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const bool has = lo[h] < hi[h];
            if (flips[h]) hold[h] = l + 1;
            rec.flips[h] = (int32_t)flips[h];
            rec.min_kept[h] = __uint_as_float(!has ? 0u : mr[h] != INT32_MAX ? mv[h] : yt[h]);
        }
        if (lane == 0) p.levels[(int64_t)b * p.L + l] = rec;
    }
    if (lane != 0) return;
    c3_subsample_window w;
    w.reads = n, w.levels_run = levels_run, w.hold_decision = hold_decision, w.reserved = 0;
    for (int h = 0; h < 4; ++h) w.hold_level[h] = hold[h];
    p.out[b] = w;
}

// ------------------------------------------------------------------------------------------ the host's plan (plain host code: tests/host/
// subsample_host_check.cpp drives it against buffers of exactly these sizes)
struct SubsamplePlan {  // what the call names, checked by the entries
    int32_t depths[kSubsampleMaxLevels] = {};
    int levels = 0, replicates = 0;
    uint64_t seed = 0;
    int64_t variants_of(int32_t n) const {  // R per level with D_l < n
        int64_t v = 0;
        for (int l = 0; l < levels; ++l) v += depths[l] < n ? replicates : 0;
        return v;
    }
};
// The pass, its cut and its layout are c3_variants.h's
static inline int64_t subsample_chunk_env() { return variant_chunk_env("C3HIP_SUBSAMPLE_CHUNK", 64); }  // windows per pass, 0 = never cut
static inline std::vector<VariantPass> subsample_cut(const int32_t *count, int64_t batch, int64_t chunk, const SubsamplePlan &plan) {
    return variant_cut(count, batch, chunk, [count, &plan](int64_t w) { return plan.variants_of(count[w]); });
}
// meta block: table | var_first | count (RunMeta); home: the 48-byte level records [windows][levels], then the 32-byte window records;
// extra: the masks of every dense window
static inline VariantLayout subsample_layout(const VariantPass &ps, size_t row_bytes, int row_floats, int levels, bool masks) {
    return VariantLayout(ps, row_bytes, RunMeta(ps, sizeof(SubsampleEntry)).bytes, row_floats,
                         (size_t)ps.windows * (levels * sizeof(c3_subsample_level) + sizeof(c3_subsample_window)),
                         masks ? (size_t)ps.dense() * 2 * sizeof(uint64_t) : 0);
}
// the meta block of a pass as it is staged, into `meta` of RunMeta(..).bytes bytes: the table (the plain windows first, then every window's
// variants in the rule's order), every window's first variant (within the pass) and its count.  first[] / count[] are the call's, checked by
// the entry
static inline void subsample_fill_pass(char *meta, const VariantPass &ps, const int32_t *first, const int32_t *count, int depth, size_t row_bytes,
                                       int layout, const SubsamplePlan &plan) {
    const RunMeta M(ps, sizeof(SubsampleEntry));
    memset(meta, 0, M.bytes);  // (the gaps between the sections)
    SubsampleEntry *tab = reinterpret_cast<SubsampleEntry *>(meta);
    int64_t *var_first = reinterpret_cast<int64_t *>(meta + M.var_first_at);
    int32_t *cnt = reinterpret_cast<int32_t *>(meta + M.count_at);
    int64_t row = 0, var = 0;
    for (int64_t i = 0; i < ps.windows; ++i) {
        const int32_t n = count[ps.w0 + i], f = first[ps.w0 + i];
        const int64_t src = row * (int64_t)row_bytes;
        tab[i] = SubsampleEntry{src, ps.w0 + i, f, n, n, 0};
        var_first[i] = var, cnt[i] = n;
        for (int l = 0; l < plan.levels; ++l) {
            const int32_t k = plan.depths[l];
            if (k >= n) continue;  // k == n: not run
            for (int32_t r = 0; r < plan.replicates; ++r)
                tab[ps.windows + var++] = SubsampleEntry{src, ps.w0 + i, layout == C3_JACKKNIFE_IN_PLACE ? f : (depth - k) / 2, n, k, r};
        }
        row += n;
    }
}
// the selection of entry e on the host, as subsample_expand_kernel makes it: src_row[d] is the read at kept slot d (for tests and the host
// check; the entries never call it)
static inline std::vector<int32_t> subsample_select(const SubsampleEntry &e, const SubsamplePlan &plan, int depth) {
    std::vector<int32_t> out;
    for (int32_t j = 0; j < e.count; ++j) {
        const uint64_t k = subsample_key(plan.seed, (uint64_t)e.window, (uint64_t)e.replicate, (uint64_t)j, (uint64_t)plan.replicates, (uint64_t)depth);
        int32_t rank = 0;
        for (int32_t i = 0; i < e.count; ++i) {
            const uint64_t o = subsample_key(plan.seed, (uint64_t)e.window, (uint64_t)e.replicate, (uint64_t)i, (uint64_t)plan.replicates, (uint64_t)depth);
            rank += o < k || (o == k && i < j);
        }
        if (e.keep >= e.count || rank < e.keep) out.push_back(j);
    }
    return out;
}

}  // namespace c3

// ------------------------------------------------------------------------------------------ the entries (include/c3hip.h)
// the mode of variant_run (c3_variants.h).  first[] / count[]: one checked entry per window (first: the base window's)
struct SubsampleMode {
    static constexpr const char *chunk_var = "C3HIP_SUBSAMPLE_CHUNK";
    c3_model *m;
    const int32_t *first, *count;
    const SubsamplePlan &plan;
    int where;  // C3_JACKKNIFE_RECENTRE / _IN_PLACE
    c3_subsample_window *out;
    c3_subsample_level *levels_out;
    uint64_t *masks_out;
    size_t row_bytes() const { return (size_t)m->positions * m->C; }
    VariantLayout layout(const VariantPass &ps) const { return subsample_layout(ps, row_bytes(), m->row, plan.levels, masks_out != nullptr); }
    void fill(char *meta, const VariantPass &ps) const { subsample_fill_pass(meta, ps, first, count, m->depth, row_bytes(), where, plan); }
    int expand(hipStream_t s, VariantTimer &timer, const int8_t *rows, const char *meta, char *masks, int64_t off, int64_t n, void *dst) const {
        const SubsampleExpandParams ep{rows, (const SubsampleEntry *)meta + off, (int8_t *)dst, masks_out ? (uint64_t *)masks + off * 2 : nullptr, plan.seed,
                                       (int)n, m->positions * m->C, (int)c3_model_window_bytes(m, C3_DTYPE_I8), m->depth, plan.replicates};
        if (ep.row_bytes % 8 == 0) return variant_launch(s, &timer, subsample_expand_kernel<8>, n, kExpandThreads, ep);
        return variant_launch(s, &timer, subsample_expand_kernel<1>, n, kExpandThreads, ep);
    }
    int reduce(hipStream_t s, VariantTimer &timer, const VariantPass &ps, const VariantLayout &L, char *base) const {
        const RunMeta M(ps, sizeof(SubsampleEntry));
        float *y = (float *)(base + L.y_at);
        SubsampleReduceParams rp;
        rp.base = y, rp.variants = y + ps.windows * m->row, rp.var_first = (const int64_t *)(base + L.meta_at + M.var_first_at);
        rp.count = (const int32_t *)(base + L.meta_at + M.count_at), rp.levels = (c3_subsample_level *)(base + L.home_at);
        rp.out = (c3_subsample_window *)(rp.levels + ps.windows * plan.levels);
        memcpy(rp.depths, plan.depths, sizeof(rp.depths));
        rp.L = plan.levels, rp.R = plan.replicates, rp.stride = m->row, rp.nout = m->nout, rp.batch = (int)ps.windows;
        return variant_launch(s, &timer, subsample_reduce_kernel, rp.batch, 64, rp);
    }
    int deliver(hipStream_t s, const VariantPass &ps, const char *home, const char *masks) const {
        const size_t lev_bytes = (size_t)ps.windows * plan.levels * sizeof(c3_subsample_level);
        memcpy(levels_out + ps.w0 * plan.levels, home, lev_bytes);
        memcpy(out + ps.w0, home + lev_bytes, (size_t)ps.windows * sizeof(c3_subsample_window));
        if (!masks_out || !ps.variants) return 0;
        return d2h_staged(masks_out + ps.var0 * 2, (const uint64_t *)masks + ps.windows * 2, (size_t)ps.variants * 2 * sizeof(uint64_t), s);
    }
};

// what the call names: levels, depths, replicates, layout (every entry; refused before anything is queued)
static int subsample_plan(const char *who, const int32_t *depths, int levels, int replicates, uint64_t seed, SubsamplePlan *plan) {
    if (levels < 1 || levels > kSubsampleMaxLevels) return fail("%s: %d levels: 1 .. %d target depths", who, levels, kSubsampleMaxLevels);
    if (!depths) return fail("null buffer: depths");
    if (replicates < 1 || replicates > kSubsampleMaxReplicates) return fail("%s: %d replicates: 1 .. %d", who, replicates, kSubsampleMaxReplicates);
    for (int l = 0; l < levels; ++l) {
        if (depths[l] < 1) return fail("%s: target depth %d at level %d: every depth must be >= 1", who, depths[l], l);
        if (l && depths[l] <= depths[l - 1]) return fail("%s: the target depths must be strictly increasing (%d behind %d)", who, depths[l], depths[l - 1]);
        plan->depths[l] = depths[l];
    }
    plan->levels = levels, plan->replicates = replicates, plan->seed = seed;
    return 0;
}

// what every entry that runs the network refuses before anything is queued
static int subsample_handle(c3_model *m, const char *who) {
    TRY(variant_handle(m, who, "%s: subsample mode draws reads of full-alignment windows: a pileup window holds counts, not reads (c3_subsample_reduce serves its rows)"));
    if (m->depth > kSubsampleMaxDepth) return fail("%s: a depth of %d rows: subsample mode ranks at most %d reads", who, m->depth, kSubsampleMaxDepth);
    return 0;
}

extern "C" {

int c3_subsample_rows(c3_model *m, const void *rows_host, const int32_t *row_first, const int32_t *row_count, int64_t batch, const int32_t *depths,
                      int levels, int replicates, uint64_t seed, int layout, float *y_host, c3_subsample_window *out, c3_subsample_level *levels_out,
                      uint64_t *masks_out, float *variant_rows_out, c3_subsample_info *info) {
    TRY(subsample_handle(m, "c3_subsample_rows"));
    if (batch < 0) return fail("negative batch");
    if (layout != C3_JACKKNIFE_RECENTRE && layout != C3_JACKKNIFE_IN_PLACE)
        return fail("c3_subsample_rows: unknown layout %d (C3_JACKKNIFE_RECENTRE or C3_JACKKNIFE_IN_PLACE)", layout);
    SubsamplePlan plan;
    TRY(subsample_plan("c3_subsample_rows", depths, levels, replicates, seed, &plan));
    if (batch > 0 && (!row_count || !out || !levels_out)) return fail("null buffer: row_count / out / levels_out");
    std::vector<int32_t> first, count;
    int64_t total = 0;
    TRY(checked_runs(m, row_first, row_count, batch, &first, &count, &total));
    if (total > 0 && !rows_host) return fail("null buffer: rows");
    if (info) *info = c3_subsample_info{};
    if (batch == 0) return 0;
    const SubsampleMode mode{m, first.data(), count.data(), plan, layout, out, levels_out, masks_out};
    return variant_run(m, "c3_subsample_rows", (const int8_t *)rows_host, C3_DTYPE_I8, subsample_cut(count.data(), batch, subsample_chunk_env(), plan),
                       mode, y_host, variant_rows_out, info);
}

int c3_subsample(c3_model *m, const void *x_host, int x_dtype, int64_t batch, const int32_t *depths, int levels, int replicates, uint64_t seed,
                 int layout, float *y_host, c3_subsample_window *out, c3_subsample_level *levels_out, uint64_t *masks_out, float *variant_rows_out,
                 c3_subsample_info *info) {
    TRY(subsample_handle(m, "c3_subsample"));
    if (batch < 0) return fail("negative batch");
    if (x_dtype != C3_DTYPE_I8) return fail("full-alignment windows must be int8 (got dtype %d)", x_dtype);
    if (layout != C3_JACKKNIFE_RECENTRE && layout != C3_JACKKNIFE_IN_PLACE)
        return fail("c3_subsample: unknown layout %d (C3_JACKKNIFE_RECENTRE or C3_JACKKNIFE_IN_PLACE)", layout);
    SubsamplePlan plan;
    TRY(subsample_plan("c3_subsample", depths, levels, replicates, seed, &plan));
    if (batch > 0 && (!x_host || !out || !levels_out)) return fail("null buffer: windows / out / levels_out");
    if (info) *info = c3_subsample_info{};
    if (batch == 0) return 0;
    std::vector<int32_t> first, count;
    std::vector<int8_t> rows;
    gather_runs(m, x_host, batch, &first, &count, &rows);
    const SubsampleMode mode{m, first.data(), count.data(), plan, layout, out, levels_out, masks_out};
    return variant_run(m, "c3_subsample", rows.data(), C3_DTYPE_I8, subsample_cut(count.data(), batch, subsample_chunk_env(), plan), mode, y_host,
                       variant_rows_out, info);
}

int c3_subsample_reduce(c3_model *m, const float *base_rows, const float *variant_rows, int row_floats, const int32_t *row_count, int64_t batch,
                        const int32_t *depths, int levels, int replicates, c3_subsample_window *out, c3_subsample_level *levels_out) {
    if (!m) return fail("null model");
    if (batch < 0) return fail("negative batch");
    if (batch > INT32_MAX) return fail("c3_subsample_reduce: too many windows for one call (%lld)", (long long)batch);
    SubsamplePlan plan;
    TRY(subsample_plan("c3_subsample_reduce", depths, levels, replicates, 0, &plan));
    if (row_floats != m->nout && row_floats != m->nout + kDecodeCols)
        return fail("c3_subsample_reduce: rows of %d floats: this model has %d probabilities, %d with the decoder columns", row_floats, m->nout, m->nout + kDecodeCols);
    if (batch == 0) return 0;
    if (!base_rows || !row_count || !out || !levels_out) return fail("null buffer: base_rows / row_count / out / levels_out");
    std::vector<int64_t> var_first((size_t)batch);
    std::vector<int32_t> count((size_t)batch);
    int64_t total = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const int32_t c = table_i32(row_count, b);
        if (c < 0) return fail("window %lld: negative row_count %d", (long long)b, c);
        var_first[(size_t)b] = total, count[(size_t)b] = c, total += plan.variants_of(c);
    }
    if (total > 0 && !variant_rows) return fail("null buffer: variant_rows");
    HIP_TRY(hipSetDevice(m->device));
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t rf = (size_t)row_floats * sizeof(float);
    const size_t v_at = al((size_t)batch * rf), f_at = al(v_at + (size_t)total * rf), c_at = al(f_at + (size_t)batch * 8), l_at = al(c_at + (size_t)batch * 4);
    const size_t r_at = l_at + (size_t)batch * levels * sizeof(c3_subsample_level);
    TRY(ensure_variant_buf(m, r_at + (size_t)batch * sizeof(c3_subsample_window)));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    char *base = (char *)m->variant_dev;
    TRY(h2d_staged(base, base_rows, (size_t)batch * rf, s));
    if (total) TRY(h2d_staged(base + v_at, variant_rows, (size_t)total * rf, s));
    TRY(h2d_staged(base + f_at, var_first.data(), (size_t)batch * 8, s));
    TRY(h2d_staged(base + c_at, count.data(), (size_t)batch * 4, s));
    SubsampleReduceParams rp;
    rp.base = (const float *)base, rp.variants = (const float *)(base + v_at), rp.var_first = (const int64_t *)(base + f_at);
    rp.count = (const int32_t *)(base + c_at), rp.levels = (c3_subsample_level *)(base + l_at), rp.out = (c3_subsample_window *)(base + r_at);
    memcpy(rp.depths, plan.depths, sizeof(rp.depths));
    rp.L = levels, rp.R = replicates, rp.stride = row_floats, rp.nout = m->nout, rp.batch = (int)batch;
    TRY(variant_launch(s, nullptr, subsample_reduce_kernel, batch, 64, rp));
    TRY(d2h_staged(levels_out, base + l_at, (size_t)batch * levels * sizeof(c3_subsample_level), s));
    TRY(d2h_staged(out, base + r_at, (size_t)batch * sizeof(c3_subsample_window), s));
    return 0;
}

}  // extern "C"
