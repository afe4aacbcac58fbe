// subsample_host_check.cpp -- the host code of subsample mode (clair3_amd/csrc/c3_subsample.h) without a device: the pass cut (chunk 1, 3 and
// 0 = never), the layout of a pass in the handle's buffer, the table a pass stages -- the order of its entries, src / first / count / keep /
// window / replicate for both layouts, windows with 0 and 1 reads at the ends of a pass, the windows' first variants -- and the totals, driven
// against plain host buffers that are exactly as large as the plan says, so that a byte read or written outside them is an error under
// AddressSanitizer; the host's own selection (subsample_select, the kernel's rank written for the host) is compared with a sort of (key, j),
// and the window every entry names is rebuilt byte by byte and compared with a loop; the hash's known answers; and the entries' refusals.
// Stand-alone, host only, built and run as tests/host/jackknife_host_check.cpp is:
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -DC3HIP_SRC_HASH='"host-check"' tests/host/subsample_host_check.cpp -o subsample_host_check && ./subsample_host_check
//
// (the library's one translation unit, so the device code is compiled along; it is not run.)  No HIP call is made and no device is needed.
#include "../../clair3_amd/csrc/c3_model.hip"

#include <algorithm>
#include <cstdio>

using namespace c3;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) ++failures, fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    } while (0)

// what subsample_expand_kernel writes for entry e, byte by byte on the host: zero outside rows [first, first + kept), the kept source rows
// in read order inside
static std::vector<int8_t> expand(const SubsampleEntry &e, const std::vector<int32_t> &kept, const std::vector<int8_t> &rows, int depth, size_t row_bytes) {
    std::vector<int8_t> w((size_t)depth * row_bytes, 0);
    for (size_t d = 0; d < kept.size(); ++d) {
        const size_t src = (size_t)e.src + (size_t)kept[d] * row_bytes, dst = ((size_t)e.first + d) * row_bytes;
        CHECK(src + row_bytes <= rows.size() && dst + row_bytes <= w.size());
        if (src + row_bytes <= rows.size() && dst + row_bytes <= w.size()) memcpy(w.data() + dst, rows.data() + src, row_bytes);
    }
    return w;
}

// the rule by a sort: the k reads of smallest (key, j), in read order
static std::vector<int32_t> sorted_selection(const SubsamplePlan &plan, int64_t w, int32_t r, int32_t n, int32_t k, int depth) {
    std::vector<std::pair<uint64_t, int32_t>> keyed;
    for (int32_t j = 0; j < n; ++j) keyed.push_back({subsample_key(plan.seed, (uint64_t)w, (uint64_t)r, (uint64_t)j, (uint64_t)plan.replicates, (uint64_t)depth), j});
    std::sort(keyed.begin(), keyed.end());
    std::vector<int32_t> kept;
    for (int32_t i = 0; i < k && i < n; ++i) kept.push_back(keyed[(size_t)i].second);
    std::sort(kept.begin(), kept.end());
    return kept;
}

static void one_call(int depth, size_t row_bytes, int row_floats, const std::vector<int32_t> &count, bool explicit_first, int64_t chunk, int layout,
                     const SubsamplePlan &plan) {
    const int64_t batch = (int64_t)count.size();
    std::vector<int32_t> first(count.size());
    int64_t total = 0, total_variants = 0;
    for (size_t b = 0; b < count.size(); ++b) {
        first[b] = explicit_first ? (b % 2 ? depth - count[b] : 0) : (depth - count[b]) / 2;
        total += count[b];
        for (int l = 0; l < plan.levels; ++l) total_variants += plan.depths[l] < count[b] ? plan.replicates : 0;
        int64_t mine = 0;
        for (int l = 0; l < plan.levels; ++l) mine += plan.depths[l] < count[b] ? plan.replicates : 0;
        CHECK(plan.variants_of(count[b]) == mine);
    }
    std::vector<int8_t> rows((size_t)total * row_bytes);  // row r holds r + 1 in every byte (mod 127): a row names itself
    for (int64_t r = 0; r < total; ++r) memset(rows.data() + (size_t)r * row_bytes, (int)(r % 127) + 1, row_bytes);
    const std::vector<VariantPass> passes = subsample_cut(count.data(), batch, chunk, plan);
    // the cut: the passes tile the call, `chunk` windows each but the last, a window's variants in one pass
    CHECK((int64_t)passes.size() == (batch == 0 ? 0 : chunk > 0 ? (batch + chunk - 1) / chunk : 1));
    int64_t w = 0, row = 0, variants = 0;
    for (size_t k = 0; k < passes.size(); ++k) {
        const VariantPass &ps = passes[k];
        CHECK(ps.w0 == w && ps.unit0 == row && ps.var0 == variants && ps.windows > 0 && (chunk == 0 || ps.windows <= chunk));
        CHECK(k + 1 == passes.size() || chunk == 0 || ps.windows == chunk);
        int64_t my_rows = 0, my_variants = 0;
        for (int64_t i = 0; i < ps.windows; ++i) my_rows += count[(size_t)(ps.w0 + i)], my_variants += plan.variants_of(count[(size_t)(ps.w0 + i)]);
        CHECK(ps.units == my_rows && ps.variants == my_variants && ps.dense() == ps.windows + my_variants);
        // the layout: sections that do not overlap, in order, 256-aligned, inside the allocation
        for (bool masks : {false, true}) {
            const VariantLayout L = subsample_layout(ps, row_bytes, row_floats, plan.levels, masks);
            const RunMeta M(ps, sizeof(SubsampleEntry));  // (offsets within the meta block, which starts at a multiple of 256 bytes)
            const size_t lev_at = L.home_at, rec_at = lev_at + (size_t)ps.windows * plan.levels * sizeof(c3_subsample_level);  // home: levels, then windows
            CHECK(L.in_at == 0 && L.unit_bytes == row_bytes && L.meta_at >= (size_t)ps.units * row_bytes && L.meta_at % 256 == 0);
            CHECK(M.var_first_at >= (size_t)ps.dense() * sizeof(SubsampleEntry) && (L.meta_at + M.var_first_at) % 256 == 0);
            CHECK(M.count_at >= M.var_first_at + (size_t)ps.windows * 8 && (L.meta_at + M.count_at) % 256 == 0 && L.meta_end == L.meta_at + M.count_at + (size_t)ps.windows * 4);
            CHECK(L.y_at >= L.meta_end && L.y_at % 256 == 0 && lev_at >= L.y_at + (size_t)ps.dense() * row_floats * 4 && lev_at % 256 == 0);
            CHECK(L.home_bytes == (size_t)ps.windows * (plan.levels * sizeof(c3_subsample_level) + sizeof(c3_subsample_window)));
            CHECK(L.flag_at == rec_at + (size_t)ps.windows * sizeof(c3_subsample_window) && L.extra_at >= L.flag_at + 4 && L.extra_at % 256 == 0);
            CHECK(L.bytes == L.extra_at + (masks ? (size_t)ps.dense() * 16 : 0) && L.meta_bytes == L.meta_end - L.meta_at && L.meta_bytes == M.bytes);
        }
        // the meta block, into a buffer of exactly its size
        const VariantLayout L = subsample_layout(ps, row_bytes, row_floats, plan.levels, false);
        const RunMeta M(ps, sizeof(SubsampleEntry));
        std::vector<char> meta(L.meta_bytes);
        subsample_fill_pass(meta.data(), ps, first.data(), count.data(), depth, row_bytes, layout, plan);
        const SubsampleEntry *tab = (const SubsampleEntry *)meta.data();
        const int64_t *var_first = (const int64_t *)(meta.data() + M.var_first_at);
        const int32_t *cnt = (const int32_t *)(meta.data() + M.count_at);
        const std::vector<int8_t> staged(rows.begin() + (ptrdiff_t)((size_t)ps.unit0 * row_bytes), rows.begin() + (ptrdiff_t)((size_t)(ps.unit0 + ps.units) * row_bytes));
        int64_t var = 0, r0 = 0;
        for (int64_t i = 0; i < ps.windows; ++i) {
            const int64_t win = ps.w0 + i;
            const int32_t n = count[(size_t)win], f = first[(size_t)win];
            // the plain windows first, in window order
            CHECK(tab[i].src == r0 * (int64_t)row_bytes && tab[i].window == win && tab[i].first == f && tab[i].count == n && tab[i].keep == n && tab[i].replicate == 0);
            CHECK(var_first[i] == var && cnt[i] == n);
            std::vector<int32_t> all = subsample_select(tab[i], plan, depth);
            CHECK((int32_t)all.size() == n);
            const std::vector<int8_t> base = expand(tab[i], all, staged, depth, row_bytes);
            for (int r = 0; r < depth; ++r) {  // the window of c3_predict_rows: row f + k is source row r0 + k
                const bool in = r >= f && r < f + n;
                CHECK(base[(size_t)r * row_bytes] == (in ? (int8_t)((ps.unit0 + r0 + r - f) % 127 + 1) : 0) && base[(size_t)r * row_bytes + row_bytes - 1] == base[(size_t)r * row_bytes]);
            }
            // ... then every window's variants: level by level (only levels below its count), replicate by replicate
            std::vector<std::vector<int32_t>> smaller((size_t)plan.replicates);  // the replicate's subset at the level before: nested
            for (int l = 0; l < plan.levels; ++l) {
                const int32_t keep = plan.depths[l];
                if (keep >= n) continue;
                for (int32_t r = 0; r < plan.replicates; ++r) {
                    const SubsampleEntry &e = tab[ps.windows + var];
                    const int32_t want_first = layout == C3_JACKKNIFE_IN_PLACE ? f : (depth - keep) / 2;
                    CHECK(e.src == tab[i].src && e.window == win && e.first == want_first && e.count == n && e.keep == keep && e.replicate == r);
                    CHECK(e.first >= 0 && e.first + keep <= depth);
                    const std::vector<int32_t> kept = subsample_select(e, plan, depth);
                    CHECK(kept == sorted_selection(plan, win, r, n, keep, depth) && (int32_t)kept.size() == keep);
                    CHECK(std::includes(kept.begin(), kept.end(), smaller[(size_t)r].begin(), smaller[(size_t)r].end()));
                    smaller[(size_t)r] = kept;
                    const std::vector<int8_t> v = expand(e, kept, staged, depth, row_bytes);
                    size_t d = 0;  // the kept rows, in read order, from want_first on; zero everywhere else
                    for (int q = 0; q < depth; ++q) {
                        const bool in = q >= want_first && q < want_first + keep;
                        CHECK(v[(size_t)q * row_bytes] == (in ? (int8_t)((ps.unit0 + r0 + kept[d]) % 127 + 1) : 0));
                        CHECK(v[(size_t)q * row_bytes + row_bytes - 1] == v[(size_t)q * row_bytes]);
                        d += in;
                    }
                    ++var;
                }
            }
            CHECK(var - var_first[i] == plan.variants_of(n));
            r0 += n;
        }
        CHECK(var == ps.variants && r0 == ps.units);
        w += ps.windows, row += ps.units, variants += ps.variants;
    }
    CHECK(w == batch && row == total && variants == total_variants);
}

// the cut does not show: a window's entries name the same (window, replicate, keep) whatever the chunk
static void cut_does_not_show(int depth, size_t row_bytes, const std::vector<int32_t> &count, const SubsamplePlan &plan) {
    std::vector<int32_t> first(count.size());
    for (size_t b = 0; b < count.size(); ++b) first[b] = (depth - count[b]) / 2;
    std::vector<std::vector<std::vector<int32_t>>> seen;
    for (int64_t chunk : {0, 1, 3}) {
        std::vector<std::vector<int32_t>> mine;
        for (const VariantPass &ps : subsample_cut(count.data(), (int64_t)count.size(), chunk, plan)) {
            std::vector<char> meta(subsample_layout(ps, row_bytes, 90, plan.levels, false).meta_bytes);
            subsample_fill_pass(meta.data(), ps, first.data(), count.data(), depth, row_bytes, C3_JACKKNIFE_RECENTRE, plan);
            const SubsampleEntry *tab = (const SubsampleEntry *)meta.data();
            for (int64_t v = 0; v < ps.variants; ++v) mine.push_back(subsample_select(tab[ps.windows + v], plan, depth));
        }
        seen.push_back(mine);
    }
    CHECK(seen[0] == seen[1] && seen[0] == seen[2] && !seen[0].empty());
}

static void entries(c3_model *pileup, c3_model *fa) {
    c3_subsample_window rec[2];
    c3_subsample_level lev[16];
    c3_subsample_info info;
    int8_t rows[8] = {};
    int32_t count[2] = {1, 1}, first[2] = {0, 0}, depths[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    float y[4] = {};
    CHECK(c3_subsample_rows(nullptr, rows, nullptr, count, 1, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_subsample(nullptr, rows, C3_DTYPE_I8, 1, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_subsample_reduce(nullptr, y, y, 24, count, 1, depths, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "null model"));
    auto rows_call = [&](c3_model *m, int64_t batch, const int32_t *d, int levels, int replicates, int layout) {
        return c3_subsample_rows(m, rows, nullptr, count, batch, d, levels, replicates, 7, layout, nullptr, rec, lev, nullptr, nullptr, &info);
    };
    auto dense_call = [&](c3_model *m, int64_t batch, const int32_t *d, int levels, int replicates, int layout) {
        return c3_subsample(m, rows, C3_DTYPE_I8, batch, d, levels, replicates, 7, layout, nullptr, rec, lev, nullptr, nullptr, &info);
    };
    // a pileup handle: the two entries that run the network
    pileup->loaded = true;
    CHECK(rows_call(pileup, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "counts, not reads"));
    CHECK(dense_call(pileup, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "counts, not reads"));
    // no weights
    fa->loaded = false;
    CHECK(rows_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "no weights"));
    CHECK(dense_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "no weights"));
    fa->loaded = true;
    // a submit pending on any slot, an exact-answer handle, a handle deeper than a workgroup ranks
    for (int k = 0; k < kHostSlots; ++k) {
        fa->slot[k].busy = true;
        CHECK(rows_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "a prediction is in flight: call c3_predict_wait first"));
        CHECK(dense_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "in flight"));
        fa->slot[k].busy = false;
    }
    fa->answer_exact = true;
    CHECK(rows_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "answers from the exact form"));
    CHECK(dense_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "answers from the exact form"));
    fa->answer_exact = false;
    const int depth = fa->depth;
    fa->depth = kSubsampleMaxDepth + 1;
    CHECK(rows_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "ranks at most 128 reads"));
    CHECK(dense_call(fa, 1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "ranks at most 128 reads"));
    fa->depth = depth;
    // the plan
    CHECK(rows_call(fa, -1, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "negative batch"));
    for (int layout : {-1, 2})
        CHECK(rows_call(fa, 1, depths, 2, 3, layout) != 0 && strstr(c3_last_error(), "unknown layout") && dense_call(fa, 1, depths, 2, 3, layout) != 0 &&
              strstr(c3_last_error(), "unknown layout"));
    const int32_t equal[2] = {4, 4}, falling[3] = {2, 5, 3}, zero[2] = {0, 4}, negative[1] = {-3};
    for (auto call : {+[](c3_model *m, const int32_t *d, int levels, int replicates, c3_subsample_window *r, c3_subsample_level *l) {
                          int8_t x[8] = {};
                          int32_t c[1] = {1};
                          return c3_subsample_rows(m, x, nullptr, c, 1, d, levels, replicates, 7, 0, nullptr, r, l, nullptr, nullptr, nullptr);
                      },
                      +[](c3_model *m, const int32_t *d, int levels, int replicates, c3_subsample_window *r, c3_subsample_level *l) {
                          int8_t x[8] = {};
                          return c3_subsample(m, x, C3_DTYPE_I8, 1, d, levels, replicates, 7, 0, nullptr, r, l, nullptr, nullptr, nullptr);
                      },
                      +[](c3_model *m, const int32_t *d, int levels, int replicates, c3_subsample_window *r, c3_subsample_level *l) {
                          float v[4] = {};
                          int32_t c[1] = {1};
                          return c3_subsample_reduce(m, v, v, m->nout, c, 1, d, levels, replicates, r, l);
                      }}) {
        CHECK(call(fa, depths, 0, 3, rec, lev) != 0 && strstr(c3_last_error(), "0 levels"));
        CHECK(call(fa, depths, 9, 3, rec, lev) != 0 && strstr(c3_last_error(), "9 levels"));
        CHECK(call(fa, nullptr, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "null buffer: depths"));
        CHECK(call(fa, equal, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "strictly increasing"));
        CHECK(call(fa, falling, 3, 3, rec, lev) != 0 && strstr(c3_last_error(), "strictly increasing"));
        CHECK(call(fa, zero, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "must be >= 1"));
        CHECK(call(fa, negative, 1, 3, rec, lev) != 0 && strstr(c3_last_error(), "must be >= 1"));
        CHECK(call(fa, depths, 2, 0, rec, lev) != 0 && strstr(c3_last_error(), "0 replicates"));
        CHECK(call(fa, depths, 2, 33, rec, lev) != 0 && strstr(c3_last_error(), "33 replicates"));
        CHECK(call(fa, depths, 2, 3, nullptr, lev) != 0 && strstr(c3_last_error(), "null buffer"));
        CHECK(call(fa, depths, 2, 3, rec, nullptr) != 0 && strstr(c3_last_error(), "null buffer"));
    }
    // buffers and runs
    CHECK(c3_subsample_rows(fa, rows, nullptr, nullptr, 1, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_subsample_rows(fa, nullptr, nullptr, count, 1, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer: rows"));
    CHECK(c3_subsample(fa, nullptr, C3_DTYPE_I8, 1, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_subsample(fa, rows, C3_DTYPE_I32, 1, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "must be int8"));
    count[1] = -1;
    CHECK(rows_call(fa, 2, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "window 1: negative row_count"));
    count[1] = fa->depth + 1;
    CHECK(rows_call(fa, 2, depths, 2, 3, 0) != 0 && strstr(c3_last_error(), "reach beyond the depth"));
    count[1] = 1, first[1] = -1;
    CHECK(c3_subsample_rows(fa, rows, first, count, 2, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "window 1: negative row_first"));
    first[1] = fa->depth;
    CHECK(c3_subsample_rows(fa, rows, first, count, 2, depths, 2, 3, 0, 0, nullptr, rec, lev, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "reach beyond the depth"));
    first[1] = 0;
    // batch == 0 launches nothing (no HIP call: there is no device here) and reports an empty call
    info.windows = 7;
    CHECK(c3_subsample_rows(fa, nullptr, nullptr, nullptr, 0, depths, 8, 32, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, &info) == 0 && info.windows == 0 && info.passes == 0);
    CHECK(c3_subsample(fa, nullptr, C3_DTYPE_I8, 0, depths, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    // the reduction alone: either kind, with or without weights
    for (c3_model *m : {pileup, fa}) {
        m->loaded = false;
        CHECK(c3_subsample_reduce(m, y, y, m->nout + 1, count, 1, depths, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "rows of"));
        CHECK(c3_subsample_reduce(m, y, y, m->nout, count, -1, depths, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "negative batch"));
        CHECK(c3_subsample_reduce(m, nullptr, y, m->nout, count, 1, depths, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "null buffer"));
        count[0] = 5;
        CHECK(c3_subsample_reduce(m, y, nullptr, m->nout, count, 1, depths, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "null buffer: variant_rows"));
        count[0] = -2;
        CHECK(c3_subsample_reduce(m, y, y, m->nout, count, 1, depths, 2, 3, rec, lev) != 0 && strstr(c3_last_error(), "negative row_count"));
        count[0] = 1;
        CHECK(c3_subsample_reduce(m, nullptr, nullptr, m->nout, nullptr, 0, depths, 2, 3, nullptr, nullptr) == 0);
    }
    CHECK(sizeof(c3_subsample_level) == 48 && sizeof(c3_subsample_window) == 32 && sizeof(c3_subsample_info) == 48 && sizeof(SubsampleEntry) == 32);
    // nothing was allocated: not by the refusals above, and never on a handle that did not call the mode
    CHECK(fa->variant_dev == nullptr && fa->variant_bytes == 0 && pileup->variant_dev == nullptr && pileup->variant_bytes == 0);
}

int main() {
    // the hash: the known answers of SplitMix64 from state 0
    CHECK(subsample_key(0, 0, 0, 0, 8, 89) == 0xE220A8397B1DCDAFull && subsample_key(0, 0, 0, 1, 8, 89) == 0x6E789E6AA1B965F4ull);
    CHECK(subsample_key(0, 0, 0, 2, 8, 89) == 0x06C45D188009454Full);
    CHECK(subsample_key(0, 1, 2, 3, 8, 89) == subsample_mix(0x9E3779B97F4A7C15ull * (1 + (1 * 8 + 2) * 89 + 3)));
    // the environment switch
    unsetenv("C3HIP_SUBSAMPLE_CHUNK");
    CHECK(subsample_chunk_env() == 64);
    setenv("C3HIP_SUBSAMPLE_CHUNK", "0", 1);
    CHECK(subsample_chunk_env() == 0);
    setenv("C3HIP_SUBSAMPLE_CHUNK", "5", 1);
    CHECK(subsample_chunk_env() == 5);
    setenv("C3HIP_SUBSAMPLE_CHUNK", "-2", 1);
    CHECK(subsample_chunk_env() == 64);
    unsetenv("C3HIP_SUBSAMPLE_CHUNK");
    // two plans: the GPU tests' four levels, and eight levels with a depth above every count and the largest seed
    SubsamplePlan plan;
    plan.levels = 4, plan.replicates = 3, plan.seed = 0x1234567890ABCDEFull;
    const int32_t d4[4] = {1, 2, 16, 60};
    memcpy(plan.depths, d4, sizeof(d4));
    SubsamplePlan deep;
    deep.levels = 8, deep.replicates = 2, deep.seed = ~0ull;
    const int32_t d8[8] = {1, 2, 3, 5, 8, 54, 88, 200};
    memcpy(deep.depths, d8, sizeof(d8));
    // depth 89 / C = 8 (264-byte rows), depth 89 / C = 9 (297), depth 55 / C = 8; counts 0 and 1 at the ends of the passes of every cut
    const struct { int depth; size_t row_bytes; int row_floats; } shapes[] = {{89, 264, 90 + kDecodeCols}, {89, 297, 90}, {55, 264, 24}};
    for (const auto &g : shapes) {
        const std::vector<std::vector<int32_t>> calls = {{}, {0}, {1}, {g.depth}, {0, 3, 1, 1, 2, 0, 0, g.depth, 1}, {1, 0, 17, 0, 1, 1, 5, 2, 0, 1}};
        for (const auto &count : calls)
            for (int64_t chunk : {1, 3, 0})
                for (int layout : {C3_JACKKNIFE_RECENTRE, C3_JACKKNIFE_IN_PLACE})
                    for (bool explicit_first : {false, true})
                        for (const SubsamplePlan *pl : {&plan, &deep}) one_call(g.depth, g.row_bytes, g.row_floats, count, explicit_first, chunk, layout, *pl);
        cut_does_not_show(g.depth, g.row_bytes, {0, 3, 17, 1, g.depth, 2, 5}, plan);
    }
    c3_model *pileup = new c3_model(), *fa = new c3_model();
    pileup->kind = C3_KIND_PILEUP, pileup->C = 18, pileup->nb = 2, pileup->nout = 24, pileup->row = 24;
    fa->kind = C3_KIND_FULL_ALIGNMENT, fa->C = 9, fa->depth = 55, fa->nb = 4, fa->nout = 90, fa->row = 90 + kDecodeCols;
    entries(pileup, fa);
    delete pileup;
    delete fa;
    printf("subsample_host_check: %d failure(s)\n", failures);
    return failures != 0;
}
