// jackknife_host_check.cpp -- the host code of jackknife mode (clair3_amd/csrc/c3_jackknife.h) without a device: the pass cut (chunk 1, 3 and
// 0 = never), the layout of a pass in the handle's buffer, the table a pass stages -- the order of its entries, src / first / count / skip for
// both layouts, counts 0 and 1 at the ends of a pass, the windows' first variants -- and the totals, driven against plain host buffers that are
// exactly as large as the plan says, so that a byte read or written outside them is an error under AddressSanitizer; the rows every entry
// names are then rebuilt on the host and compared with a loop that leaves the read out; and the entries' refusals.  Stand-alone, host only:
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -DC3HIP_SRC_HASH='"host-check"' tests/host/jackknife_host_check.cpp -o jackknife_host_check && ./jackknife_host_check
//
// (the library's one translation unit, so the device code is compiled along; it is not run.)  No HIP call is made and no device is needed.
#include "../../clair3_amd/csrc/c3_model.hip"

#include <cstdio>

using namespace c3;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) ++failures, fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    } while (0)

// what jackknife_expand_kernel writes for entry e, byte by byte on the host: zero outside the run, the source rows without row `skip` inside
static std::vector<int8_t> expand(const JackknifeEntry &e, const std::vector<int8_t> &rows, int depth, size_t row_bytes) {
    std::vector<int8_t> w((size_t)depth * row_bytes, 0);
    const int kept = e.count - (e.skip >= 0 ? 1 : 0);
    for (int r = 0; r < kept; ++r) {
        const int q = e.skip >= 0 && r >= e.skip ? r + 1 : r;
        const size_t src = (size_t)e.src + (size_t)q * row_bytes, dst = (size_t)(e.first + r) * row_bytes;
        CHECK(src + row_bytes <= rows.size() && dst + row_bytes <= w.size());
        if (src + row_bytes <= rows.size() && dst + row_bytes <= w.size()) memcpy(w.data() + dst, rows.data() + src, row_bytes);
    }
    return w;
}

static void one_call(int depth, size_t row_bytes, int row_floats, const std::vector<int32_t> &count, bool explicit_first, int64_t chunk, int layout) {
    const int64_t batch = (int64_t)count.size();
    std::vector<int32_t> first(count.size());
    int64_t total = 0;
    for (size_t b = 0; b < count.size(); ++b) {
        first[b] = explicit_first ? (b % 2 ? depth - count[b] : 0) : (depth - count[b]) / 2;
        total += count[b];
    }
    std::vector<int8_t> rows((size_t)total * row_bytes);  // row r holds r + 1 in every byte (mod 127): a row names itself
    for (int64_t r = 0; r < total; ++r) memset(rows.data() + (size_t)r * row_bytes, (int)(r % 127) + 1, row_bytes);
    const std::vector<VariantPass> passes = jackknife_cut(count.data(), batch, chunk);
    // the cut: the passes tile the call, `chunk` windows each but the last, a window's variants in one pass
    CHECK((int64_t)passes.size() == (batch == 0 ? 0 : chunk > 0 ? (batch + chunk - 1) / chunk : 1));
    int64_t w = 0, row = 0, variants = 0;
    for (size_t k = 0; k < passes.size(); ++k) {
        const VariantPass &ps = passes[k];
        CHECK(ps.w0 == w && ps.unit0 == row && ps.var0 == row && ps.windows > 0 && (chunk == 0 || ps.windows <= chunk));
        CHECK(k + 1 == passes.size() || chunk == 0 || ps.windows == chunk);
        int64_t mine = 0;
        for (int64_t i = 0; i < ps.windows; ++i) mine += count[(size_t)(ps.w0 + i)];
        CHECK(ps.units == mine && ps.variants == mine && ps.dense() == ps.windows + mine);
        // the layout: sections that do not overlap, in order, 256-aligned, inside the allocation
        for (bool drops : {false, true}) {
            const VariantLayout L = jackknife_layout(ps, row_bytes, row_floats, drops);
            const RunMeta M(ps, sizeof(JackknifeEntry));  // (offsets within the meta block, which starts at a multiple of 256 bytes)
            CHECK(L.in_at == 0 && L.unit_bytes == row_bytes && L.meta_at >= (size_t)ps.units * row_bytes && L.meta_at % 256 == 0);
            CHECK(M.var_first_at >= (size_t)ps.dense() * sizeof(JackknifeEntry) && (L.meta_at + M.var_first_at) % 256 == 0);
            CHECK(M.count_at >= M.var_first_at + (size_t)ps.windows * 8 && (L.meta_at + M.count_at) % 256 == 0 && L.meta_end == L.meta_at + M.count_at + (size_t)ps.windows * 4);
            CHECK(L.y_at >= L.meta_end && L.y_at % 256 == 0 && L.home_at >= L.y_at + (size_t)ps.dense() * row_floats * 4 && L.home_at % 256 == 0);
            CHECK(L.flag_at == L.home_at + (size_t)ps.windows * sizeof(c3_jackknife_window) && L.extra_at >= L.flag_at + 4 && L.extra_at % 256 == 0);
            CHECK(L.bytes == L.extra_at + (drops ? (size_t)ps.variants * 16 : 0) && L.meta_bytes == L.meta_end - L.meta_at && L.meta_bytes == M.bytes);
        }
        // the meta block, into a buffer of exactly its size
        const VariantLayout L = jackknife_layout(ps, row_bytes, row_floats, false);
        const RunMeta M(ps, sizeof(JackknifeEntry));
        std::vector<char> meta(L.meta_bytes);
        jackknife_fill_pass(meta.data(), ps, first.data(), count.data(), depth, row_bytes, layout);
        const JackknifeEntry *tab = (const JackknifeEntry *)meta.data();
        const int64_t *var_first = (const int64_t *)(meta.data() + M.var_first_at);
        const int32_t *cnt = (const int32_t *)(meta.data() + M.count_at);
        const std::vector<int8_t> staged(rows.begin() + (ptrdiff_t)((size_t)ps.unit0 * row_bytes), rows.begin() + (ptrdiff_t)((size_t)(ps.unit0 + ps.units) * row_bytes));
        int64_t var = 0, r0 = 0;
        for (int64_t i = 0; i < ps.windows; ++i) {
            const int32_t n = count[(size_t)(ps.w0 + i)], f = first[(size_t)(ps.w0 + i)];
            // base entries first, in window order
            CHECK(tab[i].src == r0 * (int64_t)row_bytes && tab[i].first == f && tab[i].count == n && tab[i].skip == -1 && tab[i].pad == 0);
            CHECK(var_first[i] == var && cnt[i] == n);
            const std::vector<int8_t> base = expand(tab[i], staged, depth, row_bytes);
            for (int r = 0; r < depth; ++r) {  // the window of c3_predict_rows: row f + k is source row r0 + k
                const bool in = r >= f && r < f + n;
                CHECK(base[(size_t)r * row_bytes] == (in ? (int8_t)((ps.unit0 + r0 + r - f) % 127 + 1) : 0) && base[(size_t)r * row_bytes + row_bytes - 1] == base[(size_t)r * row_bytes]);
            }
            // ... then every window's variants in window order, read order
            for (int32_t j = 0; j < n; ++j) {
                const JackknifeEntry &e = tab[ps.windows + var + j];
                const int32_t want_first = layout == C3_JACKKNIFE_IN_PLACE ? f : (depth - (n - 1)) / 2;
                CHECK(e.src == tab[i].src && e.first == want_first && e.count == n && e.skip == j && e.pad == 0);
                CHECK(e.first >= 0 && e.first + (n - 1) <= depth);
                const std::vector<int8_t> v = expand(e, staged, depth, row_bytes);
                int k = 0;  // the rows that stay, in order, from want_first on; zero everywhere else
                for (int r = 0; r < depth; ++r) {
                    const bool in = r >= want_first && r < want_first + n - 1;
                    if (in && k == j) ++k;
                    CHECK(v[(size_t)r * row_bytes] == (in ? (int8_t)((ps.unit0 + r0 + k) % 127 + 1) : 0));
                    k += in;
                }
                if (n == 1) CHECK(std::all_of(v.begin(), v.end(), [](int8_t x) { return x == 0; }));  // the all-zero window
            }
            var += n, r0 += n;
        }
        CHECK(var == ps.variants && r0 == ps.units);
        w += ps.windows, row += ps.units, variants += ps.variants;
    }
    CHECK(w == batch && row == total && variants == total);
}

static void entries(c3_model *pileup, c3_model *fa) {
    c3_jackknife_window rec[2];
    c3_jackknife_info info;
    int8_t rows[8] = {};
    int32_t count[2] = {1, 1}, first[2] = {0, 0};
    float y[4] = {};
    CHECK(c3_jackknife_rows(nullptr, rows, nullptr, count, 1, 0, nullptr, rec, nullptr, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_jackknife(nullptr, rows, C3_DTYPE_I8, 1, 0, nullptr, rec, nullptr, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_jackknife_reduce(nullptr, y, y, 24, count, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    // a pileup handle: the two entries that run the network
    pileup->loaded = true;
    CHECK(c3_jackknife_rows(pileup, rows, nullptr, count, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "counts, not reads"));
    CHECK(c3_jackknife(pileup, rows, C3_DTYPE_I8, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "counts, not reads"));
    // no weights
    fa->loaded = false;
    CHECK(c3_jackknife_rows(fa, rows, nullptr, count, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "no weights"));
    CHECK(c3_jackknife(fa, rows, C3_DTYPE_I8, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "no weights"));
    fa->loaded = true;
    // a submit pending on any slot, an exact-answer handle
    for (int k = 0; k < kHostSlots; ++k) {
        fa->slot[k].busy = true;
        CHECK(c3_jackknife_rows(fa, rows, nullptr, count, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "a prediction is in flight: call c3_predict_wait first"));
        CHECK(c3_jackknife(fa, rows, C3_DTYPE_I8, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "in flight"));
        fa->slot[k].busy = false;
    }
    fa->answer_exact = true;
    CHECK(c3_jackknife_rows(fa, rows, nullptr, count, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "answers from the exact form"));
    CHECK(c3_jackknife(fa, rows, C3_DTYPE_I8, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "answers from the exact form"));
    fa->answer_exact = false;
    // arguments
    CHECK(c3_jackknife_rows(fa, rows, nullptr, count, -1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "negative batch"));
    for (int layout : {-1, 2})
        CHECK(c3_jackknife_rows(fa, rows, nullptr, count, 1, layout, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "unknown layout") &&
              c3_jackknife(fa, rows, C3_DTYPE_I8, 1, layout, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "unknown layout"));
    CHECK(c3_jackknife_rows(fa, rows, nullptr, nullptr, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_jackknife_rows(fa, rows, nullptr, count, 1, 0, nullptr, nullptr, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_jackknife_rows(fa, nullptr, nullptr, count, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer: rows"));
    CHECK(c3_jackknife(fa, nullptr, C3_DTYPE_I8, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_jackknife(fa, rows, C3_DTYPE_I8, 1, 0, nullptr, nullptr, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_jackknife(fa, rows, C3_DTYPE_I32, 1, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "must be int8"));
    count[1] = -1;
    CHECK(c3_jackknife_rows(fa, rows, nullptr, count, 2, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "window 1: negative row_count"));
    count[1] = fa->depth + 1;
    CHECK(c3_jackknife_rows(fa, rows, nullptr, count, 2, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "reach beyond the depth"));
    count[1] = 1, first[1] = -1;
    CHECK(c3_jackknife_rows(fa, rows, first, count, 2, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "window 1: negative row_first"));
    first[1] = fa->depth;
    CHECK(c3_jackknife_rows(fa, rows, first, count, 2, 0, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "reach beyond the depth"));
    first[1] = 0;
    // batch == 0 launches nothing (no HIP call: there is no device here) and reports an empty call
    info.windows = 7;
    CHECK(c3_jackknife_rows(fa, nullptr, nullptr, nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, &info) == 0 && info.windows == 0 && info.passes == 0);
    CHECK(c3_jackknife(fa, nullptr, C3_DTYPE_I8, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    // the reduction alone: either kind, with or without weights
    for (c3_model *m : {pileup, fa}) {
        m->loaded = false;
        CHECK(c3_jackknife_reduce(m, y, y, m->nout + 1, count, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "rows of"));
        CHECK(c3_jackknife_reduce(m, y, y, m->nout, count, -1, rec, nullptr) != 0 && strstr(c3_last_error(), "negative batch"));
        CHECK(c3_jackknife_reduce(m, nullptr, y, m->nout, count, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "null buffer"));
        CHECK(c3_jackknife_reduce(m, y, y, m->nout + kDecodeCols, count, 1, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null buffer"));
        CHECK(c3_jackknife_reduce(m, y, nullptr, m->nout, count, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "null buffer: variant_rows"));
        count[0] = -2;
        CHECK(c3_jackknife_reduce(m, y, y, m->nout, count, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "negative row_count"));
        count[0] = 1;
        CHECK(c3_jackknife_reduce(m, nullptr, nullptr, m->nout, nullptr, 0, nullptr, nullptr) == 0);
    }
    CHECK(sizeof(c3_jackknife_window) == 80 && sizeof(c3_jackknife_info) == 48 && sizeof(JackknifeEntry) == 24);
    CHECK(fa->variant_dev == nullptr && fa->variant_bytes == 0 && pileup->variant_dev == nullptr);  // nothing was allocated
}

int main() {
    // the environment switch
    unsetenv("C3HIP_JACKKNIFE_CHUNK");
    CHECK(jackknife_chunk_env() == 64);
    setenv("C3HIP_JACKKNIFE_CHUNK", "0", 1);
    CHECK(jackknife_chunk_env() == 0);
    setenv("C3HIP_JACKKNIFE_CHUNK", "5", 1);
    CHECK(jackknife_chunk_env() == 5);
    unsetenv("C3HIP_JACKKNIFE_CHUNK");
    // depth 89 / C = 8 (264-byte rows), depth 89 / C = 9 (297), depth 55 / C = 8; counts 0 and 1 at the ends of the passes of every cut
    const struct { int depth; size_t row_bytes; int row_floats; } shapes[] = {{89, 264, 90 + kDecodeCols}, {89, 297, 90}, {55, 264, 24}};
    for (const auto &g : shapes) {
        const std::vector<std::vector<int32_t>> calls = {{}, {0}, {1}, {g.depth}, {0, 3, 1, 1, 2, 0, 0, g.depth, 1}, {1, 0, 17, 0, 1, 1, 5, 2, 0, 1}};
        for (const auto &count : calls)
            for (int64_t chunk : {1, 3, 0})
                for (int layout : {C3_JACKKNIFE_RECENTRE, C3_JACKKNIFE_IN_PLACE})
                    for (bool explicit_first : {false, true}) one_call(g.depth, g.row_bytes, g.row_floats, count, explicit_first, chunk, layout);
    }
    c3_model *pileup = new c3_model(), *fa = new c3_model();
    pileup->kind = C3_KIND_PILEUP, pileup->C = 18, pileup->nb = 2, pileup->nout = 24, pileup->row = 24;
    fa->kind = C3_KIND_FULL_ALIGNMENT, fa->C = 9, fa->depth = 55, fa->nb = 4, fa->nout = 90, fa->row = 90 + kDecodeCols;
    entries(pileup, fa);
    delete pileup;
    delete fa;
    printf("jackknife_host_check: %d failure(s)\n", failures);
    return failures != 0;
}
