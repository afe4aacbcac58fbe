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
// A call is cut into passes of `chunk` windows (0: one pass); a window's variants never straddle a pass.
struct SubsamplePass {
    int64_t w0 = 0, windows = 0;     // the windows [w0, w0 + windows) of the call
    int64_t row0 = 0, rows = 0;      // their occupied rows in the caller's rows: [row0, row0 + rows)
    int64_t var0 = 0, variants = 0;  // their variants among the call's: [var0, var0 + variants)
    int64_t dense() const { return windows + variants; }  // dense windows the pass builds: base windows first, then every variant
};
static inline int64_t subsample_chunk_env() {  // env C3HIP_SUBSAMPLE_CHUNK: windows per pass, default 64, 0 = never cut
    const char *e = getenv("C3HIP_SUBSAMPLE_CHUNK");
    const long long v = e ? atoll(e) : 64;
    return v < 0 ? 64 : (int64_t)v;
}
static inline std::vector<SubsamplePass> subsample_cut(const int32_t *count, int64_t batch, int64_t chunk, const SubsamplePlan &plan) {
    std::vector<SubsamplePass> out;
    int64_t row = 0, var = 0;
    for (int64_t w = 0; w < batch;) {
        SubsamplePass ps;
        ps.w0 = w, ps.windows = chunk > 0 ? std::min(chunk, batch - w) : batch - w, ps.row0 = row, ps.var0 = var;
        for (int64_t i = 0; i < ps.windows; ++i) ps.rows += count[w + i], ps.variants += plan.variants_of(count[w + i]);
        out.push_back(ps);
        w += ps.windows, row += ps.rows, var += ps.variants;
    }
    return out;
}
// where a pass's sections sit in the handle's subsample buffer (every section from a multiple of 256 bytes)
struct SubsampleLayout {
    size_t rows_at = 0, tab_at = 0, var_first_at = 0, count_at = 0;  // staged: the occupied rows; then the meta block [tab_at, meta_end)
    size_t meta_end = 0;
    size_t y_at = 0, lev_at = 0, rec_at = 0, flag_at = 0, masks_at = 0, bytes = 0;  // written by the device
    SubsampleLayout(const SubsamplePass &ps, size_t row_bytes, int row_floats, int levels, bool masks) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        tab_at = al((size_t)ps.rows * row_bytes);
        var_first_at = al(tab_at + (size_t)ps.dense() * sizeof(SubsampleEntry));
        count_at = al(var_first_at + (size_t)ps.windows * sizeof(int64_t));
        meta_end = count_at + (size_t)ps.windows * sizeof(int32_t);
        y_at = al(meta_end);
        lev_at = al(y_at + (size_t)ps.dense() * row_floats * sizeof(float));
        rec_at = lev_at + (size_t)ps.windows * levels * sizeof(c3_subsample_level);  // (48- and 32-byte records: multiples of 4) ...
        flag_at = rec_at + (size_t)ps.windows * sizeof(c3_subsample_window);         // ... and behind them the pass's copy of the range flag
        masks_at = al(flag_at + 4);
        bytes = masks_at + (masks ? (size_t)ps.dense() * 2 * sizeof(uint64_t) : 0);
    }
    size_t meta_bytes() const { return meta_end - tab_at; }
};
// the meta block of a pass as it is staged, into `meta` of L.meta_bytes() bytes: the table (the plain windows first, then every window's
// variants in the rule's order), every window's first variant (within the pass) and its count.  first[] / count[] are the call's, checked by
// the entry
static inline void subsample_fill_pass(char *meta, const SubsampleLayout &L, const SubsamplePass &ps, const int32_t *first, const int32_t *count,
                                       int depth, size_t row_bytes, int layout, const SubsamplePlan &plan) {
    memset(meta, 0, L.meta_bytes());  // (the gaps between the sections)
    SubsampleEntry *tab = reinterpret_cast<SubsampleEntry *>(meta);
    int64_t *var_first = reinterpret_cast<int64_t *>(meta + (L.var_first_at - L.tab_at));
    int32_t *cnt = reinterpret_cast<int32_t *>(meta + (L.count_at - L.tab_at));
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
// the handle's subsample buffer: a pass's staged rows, its meta block, the rows of its dense windows, the records, the masks; grown, never shrunk
static int ensure_subsample_buf(c3_model *m, size_t bytes) {
    if (m->subsample_bytes >= bytes) return 0;
    HIP_TRY(hipDeviceSynchronize());
    if (m->subsample_dev) (void)hipFree(m->subsample_dev);
    m->subsample_dev = nullptr, m->subsample_bytes = 0;
    HIP_TRY(hipMalloc(&m->subsample_dev, bytes));
    m->subsample_bytes = bytes;
    return 0;
}

static int subsample_reduce_launch(hipStream_t s, const SubsampleReduceParams &rp, JackknifeTimer *timer = nullptr) {
    if (rp.batch <= 0) return 0;
    if (timer) timer->mark(s);
    hipLaunchKernelGGL(subsample_reduce_kernel, dim3((unsigned)rp.batch), dim3(64), 0, s, rp);
    HIP_TRY(hipGetLastError());
    if (timer) timer->mark(s);
    return 0;
}

// the dense windows of a pass, micro-batch by micro-batch through the forms the handle is on, their rows at y (row stride m->row)
static int subsample_forward(c3_model *m, hipStream_t s, const int8_t *rows, const SubsampleEntry *tab, uint64_t *masks, int64_t total, float *y,
                             const SubsamplePlan &plan, JackknifeTimer &timer) {
    TRY(ensure_workspace(m, total));
    TRY(ensure_expand_buf(m));
    Lane &L = lane(m);
    const int64_t wbytes = c3_model_window_bytes(m, C3_DTYPE_I8);
    for (int64_t off = 0; off < total; off += L.cap) {
        const int64_t n = std::min<int64_t>(L.cap, total - off);
        const SubsampleExpandParams ep{rows, tab + off, L.xe, masks ? masks + off * 2 : nullptr, plan.seed, (int)n, m->positions * m->C, (int)wbytes,
                                       m->depth, plan.replicates};
        timer.mark(s);
        if (ep.row_bytes % 8 == 0) hipLaunchKernelGGL(subsample_expand_kernel<8>, dim3((unsigned)n), dim3(kExpandThreads), 0, s, ep);
        else hipLaunchKernelGGL(subsample_expand_kernel<1>, dim3((unsigned)n), dim3(kExpandThreads), 0, s, ep);
        HIP_TRY(hipGetLastError());
        timer.mark(s);
        TRY(run_fa(m, s, L.xe, n, y + off * m->row));
        L.last_n = n;
    }
    return 0;
}

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
    if (!m) return fail("null model");
    if (m->kind != C3_KIND_FULL_ALIGNMENT)
        return fail("%s: subsample mode draws reads of full-alignment windows: a pileup window holds counts, not reads (c3_subsample_reduce serves its rows)", who);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("%s: a prediction is in flight: call c3_predict_wait first", who);
    if (m->answer_exact) return fail("%s: the handle answers from the exact form: c3_model_set_answer(m, C3_ANSWER_PRODUCT) first", who);
    if (!m->loaded) return fail("model has no weights: call c3_model_load first");
    if (m->depth > kSubsampleMaxDepth) return fail("%s: a depth of %d rows: subsample mode ranks at most %d reads", who, m->depth, kSubsampleMaxDepth);
    return 0;
}

// first[] / count[]: one checked entry per window (first: the base window's).  The pass loop is jackknife_run's (c3_jackknife.h): the forms
// the handle is on for this call alone, two attempts per pass for the range guard, one wait per pass for the records
static int subsample_run(c3_model *m, const int8_t *rows_host, const int32_t *first, const int32_t *count, int64_t batch, const SubsamplePlan &plan,
                         int layout, float *y_host, c3_subsample_window *out, c3_subsample_level *levels_out, uint64_t *masks_out,
                         float *variant_rows_out, c3_subsample_info *info) {
    HIP_TRY(hipSetDevice(m->device));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    const size_t row_bytes = (size_t)m->positions * m->C;
    const std::vector<SubsamplePass> passes = subsample_cut(count, batch, subsample_chunk_env(), plan);
    size_t need = 0;
    for (const SubsamplePass &ps : passes) {
        if (ps.dense() > INT32_MAX) return fail("c3_subsample_rows: %lld dense windows in one pass: set C3HIP_SUBSAMPLE_CHUNK", (long long)ps.dense());
        need = std::max(need, SubsampleLayout(ps, row_bytes, m->row, plan.levels, masks_out != nullptr).bytes);
    }
    TRY(ensure_subsample_buf(m, need));
    const c3_model::Choices reported = m->choice;
    const bool f16 = m->f16_ok, tap_call = m->tap_call, prof = m->prof;
    const int64_t tap_base = m->tap_base;
    const uint32_t tap_mask = m->tap_mask;
    int rc = 0, on_fp32 = 0;
    size_t staged = 0;
    JackknifeTimer t_expand, t_reduce;
    t_expand.on = t_reduce.on = info != nullptr;
    std::vector<char> meta;
    char *base = (char *)m->subsample_dev;
    for (const SubsamplePass &ps : passes) {
        const SubsampleLayout L(ps, row_bytes, m->row, plan.levels, masks_out != nullptr);
        meta.resize(L.meta_bytes());
        subsample_fill_pass(meta.data(), L, ps, first, count, m->depth, row_bytes, layout, plan);
        if (ps.rows) rc = h2d_staged(base + L.rows_at, rows_host + (size_t)ps.row0 * row_bytes, (size_t)ps.rows * row_bytes, s);
        if (rc == 0) rc = h2d_staged(base + L.tab_at, meta.data(), meta.size(), s);
        if (rc) break;
        staged += (size_t)ps.rows * row_bytes + meta.size();
        float *y = (float *)(base + L.y_at);
        uint64_t *masks = masks_out ? (uint64_t *)(base + L.masks_at) : nullptr;
        SubsampleReduceParams rp;
        rp.base = y, rp.variants = y + ps.windows * m->row, rp.var_first = (const int64_t *)(base + L.var_first_at);
        rp.count = (const int32_t *)(base + L.count_at), rp.levels = (c3_subsample_level *)(base + L.lev_at), rp.out = (c3_subsample_window *)(base + L.rec_at);
        memcpy(rp.depths, plan.depths, sizeof(rp.depths));
        rp.L = plan.levels, rp.R = plan.replicates, rp.stride = m->row, rp.nout = m->nout, rp.batch = (int)ps.windows;
        for (int attempt = 0; attempt < 2 && rc == 0; ++attempt) {
            const bool guarded = f16 && attempt == 0;  // the fp16x3 forms raise the range flag; the fp32 forms of the second attempt do not look at it
            m->f16_ok = attempt == 0 ? f16 : false, m->tap_call = true, m->prof = false, m->tap_mask = 0;
            rc = subsample_forward(m, s, (const int8_t *)(base + L.rows_at), (const SubsampleEntry *)(base + L.tab_at), masks, ps.dense(), y, plan, t_expand);
            m->f16_ok = f16, m->tap_call = tap_call, m->prof = prof, m->tap_base = tap_base, m->tap_mask = tap_mask, m->choice = reported;
            if (rc) break;
            if (guarded) {  // a non-finite row raises bit 1 of the flag as in the ring
                const int64_t nf = ps.dense() * m->row;
                hipLaunchKernelGGL(rows_finite_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, y, nf, m->range_flag);
                if (hipGetLastError() != hipSuccess) {
                    rc = fail("c3_subsample_rows: the scan of the rows could not be launched");
                    break;
                }
            }
            if ((rc = subsample_reduce_launch(s, rp, &t_reduce)) != 0) break;
            // the level records, the window records and, behind them, the pass's copy of the range flag come home in one copy
            if (hipMemcpyAsync(base + L.flag_at, m->range_flag, 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
                rc = fail("c3_subsample_rows: hipMemcpyAsync failed");
                break;
            }
            std::vector<char> home(L.flag_at + 4 - L.lev_at);
            if ((rc = d2h_staged(home.data(), base + L.lev_at, home.size(), s)) != 0) break;
            uint32_t flag = 0;
            memcpy(&flag, home.data() + home.size() - 4, 4);
            if (guarded && flag) {  // beyond the range of the fp16x3 kernels: this pass again on the fp32-MFMA forms, for this call alone
                if (hipMemsetAsync(m->range_flag, 0, 256, s) != hipSuccess) rc = fail("c3_subsample_rows: hipMemsetAsync failed");
                on_fp32 = 1;
                continue;
            }
            memcpy(levels_out + ps.w0 * plan.levels, home.data(), (size_t)ps.windows * plan.levels * sizeof(c3_subsample_level));
            memcpy(out + ps.w0, home.data() + (L.rec_at - L.lev_at), (size_t)ps.windows * sizeof(c3_subsample_window));
            if (y_host) rc = d2h_staged(y_host + ps.w0 * m->row, y, (size_t)ps.windows * m->row * sizeof(float), s);
            if (rc == 0 && masks_out && ps.variants)
                rc = d2h_staged(masks_out + ps.var0 * 2, masks + ps.windows * 2, (size_t)ps.variants * 2 * sizeof(uint64_t), s);
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
        *info = c3_subsample_info{};
        info->expand_us = expand_us, info->reduce_us = reduce_us;
        info->windows = batch, info->passes = (int64_t)passes.size(), info->bytes_staged = (int64_t)staged, info->on_fp32 = on_fp32;
        for (const SubsamplePass &ps : passes) info->variants += ps.variants;
    }
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
    if (info) *info = c3_subsample_info{};
    if (batch == 0) return 0;
    return subsample_run(m, (const int8_t *)rows_host, first.data(), count.data(), batch, plan, layout, y_host, out, levels_out, masks_out,
                         variant_rows_out, info);
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
    // every window's run, found on the host as c3_jackknife finds it; its first row is the run's own
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
    return subsample_run(m, rows.data(), first.data(), count.data(), batch, plan, layout, y_host, out, levels_out, masks_out, variant_rows_out, info);
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
    TRY(ensure_subsample_buf(m, r_at + (size_t)batch * sizeof(c3_subsample_window)));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    char *base = (char *)m->subsample_dev;
    TRY(h2d_staged(base, base_rows, (size_t)batch * rf, s));
    if (total) TRY(h2d_staged(base + v_at, variant_rows, (size_t)total * rf, s));
    TRY(h2d_staged(base + f_at, var_first.data(), (size_t)batch * 8, s));
    TRY(h2d_staged(base + c_at, count.data(), (size_t)batch * 4, s));
    SubsampleReduceParams rp;
    rp.base = (const float *)base, rp.variants = (const float *)(base + v_at), rp.var_first = (const int64_t *)(base + f_at);
    rp.count = (const int32_t *)(base + c_at), rp.levels = (c3_subsample_level *)(base + l_at), rp.out = (c3_subsample_window *)(base + r_at);
    memcpy(rp.depths, plan.depths, sizeof(rp.depths));
    rp.L = levels, rp.R = replicates, rp.stride = row_floats, rp.nout = m->nout, rp.batch = (int)batch;
    TRY(subsample_reduce_launch(s, rp));
    TRY(d2h_staged(levels_out, base + l_at, (size_t)batch * levels * sizeof(c3_subsample_level), s));
    TRY(d2h_staged(out, base + r_at, (size_t)batch * sizeof(c3_subsample_window), s));
    return 0;
}

}  // extern "C"
