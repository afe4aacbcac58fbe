// occlude_host_check.cpp -- the host code of occlusion mode (clair3_amd/csrc/c3_occlude.h) without a device: the pass cut (chunk 1, 3 and
// 0 = never), the layout of a pass in the handle's buffer and the table a pass stages -- the order of its entries, src / first / count / chan /
// col_lo / col_hi, for both kinds, C = 8, 9 and 18, band 1, 5 and P, every `what`, counts 0 and 1 at the ends of a pass --, driven against
// plain host buffers that are exactly as large as the plan says, so that a byte read or written outside them is an error under
// AddressSanitizer.  The dense window of every entry is then rebuilt on the host the way the kernels walk it -- thread by thread, piece by
// piece, channel and column kept by the additions of OccludeWalk -- and compared with a plain loop over (read, position, channel); and the
// entries' refusals that need no device.  Stand-alone, host only:
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++20 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -DC3HIP_SRC_HASH='"host-check"' tests/host/occlude_host_check.cpp -o occlude_host_check && ./occlude_host_check
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

// OccludeWalk on the host: the same additions and conditional subtractions
struct Walk {
    int c, pos, dc, dpos, C, P;
    Walk(int i0, int step, int C_, int P_) : C(C_), P(P_) { c = i0 % C, pos = (i0 / C) % P, dc = step % C, dpos = (step / C) % P; }
    void next() {
        c += dc;
        const int carry = c >= C ? 1 : 0;
        c -= carry ? C : 0;
        pos += dpos + carry;
        CHECK(pos < 2 * P);
        pos -= pos >= P ? P : 0;
    }
};

// what the expand kernels write for entry e, walked as they walk it: elements of `item` bytes (1: int8, 4: int32 pileup), `cell` = true the
// C == 8 form (a piece is a cell of 8 bytes).  units = rows per window (full alignment: depth; pileup: 1 with first = 0, count = 1)
static std::vector<int8_t> expand(const OccludeEntry &e, const std::vector<int8_t> &in, int depth, int P, int C, int item, bool cell, bool pileup) {
    const int per = cell ? 8 : item;  // bytes a piece
    const int row_pieces = P * C * item / per, n = depth * row_pieces;
    const int lo = pileup ? 0 : e.first * row_pieces, hi = pileup ? n : lo + e.count * row_pieces;
    std::vector<int8_t> w((size_t)n * per, 0x55);
    std::vector<int> written((size_t)n, 0);
    for (int tid = 0; tid < kExpandThreads; ++tid) {
        Walk k(tid, kExpandThreads, cell ? 1 : C, P);
        for (int i = tid; i < n; i += kExpandThreads, k.next()) {
            CHECK(k.pos == (i / (cell ? 1 : C)) % P && k.c == (cell ? 0 : i % C));
            ++written[(size_t)i];
            const bool in_run = i >= lo && i < hi, in_band = k.pos >= e.col_lo && k.pos < e.col_hi;
            for (int byte = 0; byte < per; ++byte) {
                const int ch = cell ? byte : k.c;
                int8_t v = 0;
                if (in_run && !in_band && ch != e.chan) {
                    const size_t src = (size_t)e.src + (size_t)(i - lo) * per + byte;
                    CHECK(src < in.size());
                    if (src < in.size()) v = in[src];
                }
                w[(size_t)i * per + byte] = v;
            }
        }
    }
    CHECK(std::all_of(written.begin(), written.end(), [](int k) { return k == 1; }));  // every piece exactly once
    return w;
}

// one call of either kind: count empty = pileup (item 1 or 4)
static void one_call(bool pileup, int depth, int P, int C, int item, int row_floats, const std::vector<int32_t> &count, bool explicit_first, int64_t chunk,
                     int what, int band) {
    const int64_t batch = (int64_t)count.size();
    const OccludePlan plan(P, C, what, band);
    const int nb = (P + band - 1) / band, K = plan.K();
    CHECK(plan.channels == (what & 1 ? C : 0) && plan.bands == (what & 2 ? nb : 0) && K >= 1);
    const size_t unit_bytes = pileup ? (size_t)P * C * item : (size_t)P * C;
    std::vector<int32_t> first(count.size());
    int64_t total = 0;
    for (size_t b = 0; b < count.size(); ++b) {
        first[b] = explicit_first ? (b % 2 ? depth - count[b] : 0) : (depth - count[b]) / 2;
        total += pileup ? 1 : count[b];
    }
    std::vector<int8_t> in((size_t)total * unit_bytes);  // every byte a non-zero function of its place: what is zero was set to zero
    for (size_t i = 0; i < in.size(); ++i) in[i] = (int8_t)(i % 125 + 1);
    const std::vector<VariantPass> passes = occlude_cut(pileup ? nullptr : count.data(), batch, chunk, K);
    CHECK((int64_t)passes.size() == (batch == 0 ? 0 : chunk > 0 ? (batch + chunk - 1) / chunk : 1));
    int64_t w = 0, unit = 0, variants = 0;
    for (size_t k = 0; k < passes.size(); ++k) {
        const VariantPass &ps = passes[k];
        CHECK(ps.w0 == w && ps.unit0 == unit && ps.var0 == w * K && ps.windows > 0 && (chunk == 0 || ps.windows <= chunk));
        CHECK(k + 1 == passes.size() || chunk == 0 || ps.windows == chunk);
        int64_t mine = 0;
        for (int64_t i = 0; i < ps.windows; ++i) mine += pileup ? 1 : count[(size_t)(ps.w0 + i)];
        CHECK(ps.units == mine && ps.variants == ps.windows * K && ps.dense() == ps.windows * (K + 1));
        // the layout: sections that do not overlap, in order, 256-aligned, inside the allocation
        for (bool drops : {false, true}) {
            const VariantLayout L = occlude_layout(ps, unit_bytes, row_floats, drops);
            CHECK(L.in_at == 0 && L.unit_bytes == unit_bytes && L.meta_at >= (size_t)ps.units * unit_bytes && L.meta_at % 256 == 0);
            CHECK(L.meta_end == L.meta_at + (size_t)ps.dense() * sizeof(OccludeEntry) && L.meta_bytes == (size_t)ps.dense() * 32);
            CHECK(L.y_at >= L.meta_end && L.y_at % 256 == 0 && L.home_at >= L.y_at + (size_t)ps.dense() * row_floats * 4 && L.home_at % 256 == 0);
            CHECK(L.flag_at == L.home_at + (size_t)ps.windows * sizeof(c3_occlude_window) && L.extra_at >= L.flag_at + 4 && L.extra_at % 256 == 0);
            CHECK(L.bytes == L.extra_at + (drops ? (size_t)ps.variants * 16 : 0));
        }
        // the table, into a buffer of exactly its size; the staged input, a buffer of exactly the pass's
        const VariantLayout L = occlude_layout(ps, unit_bytes, row_floats, false);
        std::vector<OccludeEntry> tab((size_t)ps.dense());
        CHECK(tab.size() * sizeof(OccludeEntry) == L.meta_bytes);
        occlude_fill_pass(tab.data(), ps, plan, pileup ? nullptr : first.data(), pileup ? nullptr : count.data(), unit_bytes);
        const std::vector<int8_t> staged(in.begin() + (ptrdiff_t)((size_t)ps.unit0 * unit_bytes), in.begin() + (ptrdiff_t)((size_t)(ps.unit0 + ps.units) * unit_bytes));
        const int rows = pileup ? 1 : depth;
        const bool cell = !pileup && C == 8;
        int64_t u0 = 0;
        for (int64_t i = 0; i < ps.windows; ++i) {
            const int32_t n = pileup ? 1 : count[(size_t)(ps.w0 + i)], f = pileup ? 0 : first[(size_t)(ps.w0 + i)];
            // base entries first, in window order: no mask
            const OccludeEntry &e0 = tab[(size_t)i];
            CHECK(e0.src == u0 * (int64_t)unit_bytes && e0.chan == -1 && e0.col_lo == 0 && e0.col_hi == 0 && e0.pad == 0);
            CHECK(pileup ? e0.first == 0 && e0.count == 0 : e0.first == f && e0.count == n);
            // the window itself by a plain loop over (read, position, channel) of elements
            auto plain = [&](int chan, int col_lo, int col_hi) {
                std::vector<int8_t> x((size_t)rows * P * C * item, 0);
                for (int r = 0; r < rows; ++r)
                    for (int p = 0; p < P; ++p)
                        for (int c = 0; c < C; ++c)
                            for (int byte = 0; byte < item; ++byte) {
                                const bool in_run = r >= f && r < f + n;
                                if (!in_run || c == chan || (p >= col_lo && p < col_hi)) continue;
                                const size_t src = ((size_t)(u0 + r - f) * P * C + (size_t)p * C + c) * item + byte;
                                x[(((size_t)r * P + p) * C + c) * item + byte] = staged[src];
                            }
                return x;
            };
            CHECK(expand(e0, staged, rows, P, C, item, cell, pileup) == plain(-1, 0, 0));
            if (cell) CHECK(expand(e0, staged, rows, P, C, item, false, pileup) == plain(-1, 0, 0));  // (the byte form serves C == 8 as well)
            // ... then every window's K variants in window order: channels 0 .. C - 1, then bands 0 .. nb - 1
            for (int j = 0; j < K; ++j) {
                const OccludeEntry &e = tab[(size_t)(ps.windows + i * K + j)];
                const bool is_chan = j < plan.channels;
                const int kb = j - plan.channels;
                const int want_chan = is_chan ? j : -1, want_lo = is_chan ? 0 : kb * band, want_hi = is_chan ? 0 : std::min(P, (kb + 1) * band);
                CHECK(e.src == e0.src && e.first == e0.first && e.count == e0.count && e.pad == 0);
                CHECK(e.chan == want_chan && e.col_lo == want_lo && e.col_hi == want_hi && e.chan < C && e.col_hi <= P);
                if (!is_chan) CHECK(e.col_lo < e.col_hi);
                const std::vector<int8_t> v = expand(e, staged, rows, P, C, item, cell, pileup);
                CHECK(v == plain(want_chan, want_lo, want_hi));
                if (cell) CHECK(expand(e, staged, rows, P, C, item, false, pileup) == v);
                if (n == 0 || (!is_chan && band == P)) CHECK(std::all_of(v.begin(), v.end(), [](int8_t x) { return x == 0; }));  // the zero window
            }
            if (plan.bands) CHECK(tab[(size_t)(ps.windows + i * K + K - 1)].col_hi == P && tab[(size_t)(ps.windows + i * K + plan.channels)].col_lo == 0);
            u0 += n;
        }
        CHECK(u0 == ps.units);
        w += ps.windows, unit += ps.units, variants += ps.variants;
    }
    CHECK(w == batch && unit == total && variants == batch * K);
}

static void entries(c3_model *pileup, c3_model *fa) {
    c3_occlude_window rec[2];
    c3_occlude_info info;
    int8_t rows[8] = {};
    int32_t count[2] = {1, 1}, first[2] = {0, 0};
    float y[4] = {};
    CHECK(c3_occlude(nullptr, rows, C3_DTYPE_I8, 1, 3, 1, nullptr, rec, nullptr, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_occlude_rows(nullptr, rows, nullptr, count, 1, 3, 1, nullptr, rec, nullptr, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    CHECK(c3_occlude_reduce(nullptr, y, y, 24, 1, 1, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "null model"));
    for (c3_model *m : {pileup, fa}) {
        // no weights
        m->loaded = false;
        CHECK(c3_occlude(m, rows, C3_DTYPE_I8, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "no weights"));
        CHECK(c3_occlude_rows(m, rows, nullptr, count, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "no weights"));
        m->loaded = true;
        // a submit pending on any slot, an exact-answer handle
        for (int k = 0; k < kHostSlots; ++k) {
            m->slot[k].busy = true;
            CHECK(c3_occlude(m, rows, C3_DTYPE_I8, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "a prediction is in flight: call c3_predict_wait first"));
            CHECK(c3_occlude_rows(m, rows, nullptr, count, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "in flight"));
            m->slot[k].busy = false;
        }
        m->answer_exact = true;
        CHECK(c3_occlude(m, rows, C3_DTYPE_I8, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "answers from the exact form"));
        CHECK(c3_occlude_rows(m, rows, nullptr, count, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "answers from the exact form"));
        m->answer_exact = false;
        // what, band, batch, buffers
        for (int what : {0, 4, -1})
            CHECK(c3_occlude(m, rows, C3_DTYPE_I8, 1, what, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "unknown `what`") &&
                  c3_occlude_rows(m, rows, nullptr, count, 1, what, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "unknown `what`"));
        for (int band : {0, -1, m->positions + 1})
            CHECK(c3_occlude(m, rows, C3_DTYPE_I8, 1, 3, band, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "outside 1 .. 33") &&
                  c3_occlude_rows(m, rows, nullptr, count, 1, 1, band, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "outside 1 .. 33"));
        CHECK(c3_occlude(m, rows, C3_DTYPE_I8, -1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "negative batch"));
        CHECK(c3_occlude(m, nullptr, C3_DTYPE_I8, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
        CHECK(c3_occlude(m, rows, C3_DTYPE_I8, 1, 3, 1, nullptr, nullptr, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
        // batch == 0 launches nothing (no HIP call: there is no device here) and reports an empty call
        info.windows = 7;
        CHECK(c3_occlude(m, nullptr, C3_DTYPE_I8, 0, 3, m->positions, nullptr, nullptr, nullptr, nullptr, &info) == 0 && info.windows == 0 && info.passes == 0);
    }
    // the dtype a kind takes; occupied rows are full-alignment input
    CHECK(c3_occlude(fa, rows, C3_DTYPE_I32, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "must be int8"));
    CHECK(c3_occlude(pileup, rows, C3_DTYPE_F32, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "int8 or int32"));
    CHECK(c3_occlude_rows(pileup, rows, nullptr, count, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "full-alignment input"));
    // counts and firsts that c3_predict_rows would refuse
    CHECK(c3_occlude_rows(fa, rows, nullptr, count, -1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "negative batch"));
    CHECK(c3_occlude_rows(fa, rows, nullptr, nullptr, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_occlude_rows(fa, rows, nullptr, count, 1, 3, 1, nullptr, nullptr, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer"));
    CHECK(c3_occlude_rows(fa, nullptr, nullptr, count, 1, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "null buffer: rows"));
    count[1] = -1;
    CHECK(c3_occlude_rows(fa, rows, nullptr, count, 2, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "window 1: negative row_count"));
    count[1] = fa->depth + 1;
    CHECK(c3_occlude_rows(fa, rows, nullptr, count, 2, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "reach beyond the depth"));
    count[1] = 1, first[1] = -1;
    CHECK(c3_occlude_rows(fa, rows, first, count, 2, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "window 1: negative row_first"));
    first[1] = fa->depth;
    CHECK(c3_occlude_rows(fa, rows, first, count, 2, 3, 1, nullptr, rec, nullptr, nullptr, &info) != 0 && strstr(c3_last_error(), "reach beyond the depth"));
    first[1] = 0;
    CHECK(c3_occlude_rows(fa, nullptr, nullptr, nullptr, 0, 2, 5, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    // a pass of more than INT32_MAX dense windows (never cut): refused by the plan, before any HIP call
    setenv("C3HIP_OCCLUDE_CHUNK", "0", 1);
    {
        const int64_t big = (int64_t)INT32_MAX / 52 + 1;  // x 52 dense windows a window
        const OccludePlan plan(33, 18, 3, 1);
        const std::vector<VariantPass> passes = occlude_cut(nullptr, big, occlude_chunk_env(C3_KIND_PILEUP), plan.K());
        CHECK(passes.size() == 1 && passes[0].dense() > INT32_MAX);
        std::vector<c3_occlude_window> many(1);
        const OccludeMode mode{pileup, C3_DTYPE_I8, nullptr, nullptr, plan, many.data(), nullptr};
        CHECK(variant_run(pileup, "c3_occlude", rows, C3_DTYPE_I8, passes, mode, nullptr, nullptr, nullptr) != 0 &&
              strstr(c3_last_error(), "dense windows in one pass: set C3HIP_OCCLUDE_CHUNK"));
    }
    unsetenv("C3HIP_OCCLUDE_CHUNK");
    // the reduction alone: either kind, with or without weights
    for (c3_model *m : {pileup, fa}) {
        m->loaded = false;
        CHECK(c3_occlude_reduce(m, y, y, m->nout + 1, 1, 1, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "rows of"));
        CHECK(c3_occlude_reduce(m, y, y, m->nout, 1, 1, -1, rec, nullptr) != 0 && strstr(c3_last_error(), "negative batch"));
        CHECK(c3_occlude_reduce(m, y, y, m->nout, -1, 1, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "group sizes"));
        CHECK(c3_occlude_reduce(m, y, y, m->nout, 1, -1, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "group sizes"));
        CHECK(c3_occlude_reduce(m, nullptr, y, m->nout, 1, 1, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "null buffer"));
        CHECK(c3_occlude_reduce(m, y, y, m->nout + kDecodeCols, 1, 1, 1, nullptr, nullptr) != 0 && strstr(c3_last_error(), "null buffer"));
        CHECK(c3_occlude_reduce(m, y, nullptr, m->nout, 1, 0, 1, rec, nullptr) != 0 && strstr(c3_last_error(), "null buffer: variant_rows"));
        CHECK(c3_occlude_reduce(m, nullptr, nullptr, m->nout, 8, 33, 0, nullptr, nullptr) == 0);
    }
    CHECK(sizeof(c3_occlude_window) == 144 && sizeof(c3_occlude_info) == 48 && sizeof(OccludeEntry) == 32);
    CHECK(offsetof(c3_occlude_window, flips) == 8 && offsetof(c3_occlude_window, decision_flips) == 40 && offsetof(c3_occlude_window, lean) == 72);
    CHECK(offsetof(c3_occlude_window, lean_drop) == 104 && offsetof(c3_occlude_window, max_delta) == 136 && offsetof(c3_occlude_window, reserved) == 140);
    for (c3_model *m : {pileup, fa}) {  // nothing was allocated
        CHECK(m->variant_dev == nullptr && m->variant_bytes == 0);
        for (const Lane &L : m->lanes) CHECK(L.xo == nullptr && L.xo_cap == 0);
    }
}

int main() {
    // the environment switch: read at every call, a default per kind
    unsetenv("C3HIP_OCCLUDE_CHUNK");
    CHECK(occlude_chunk_env(C3_KIND_FULL_ALIGNMENT) == 64 && occlude_chunk_env(C3_KIND_PILEUP) == 256);
    setenv("C3HIP_OCCLUDE_CHUNK", "0", 1);
    CHECK(occlude_chunk_env(C3_KIND_FULL_ALIGNMENT) == 0 && occlude_chunk_env(C3_KIND_PILEUP) == 0);
    setenv("C3HIP_OCCLUDE_CHUNK", "5", 1);
    CHECK(occlude_chunk_env(C3_KIND_FULL_ALIGNMENT) == 5 && occlude_chunk_env(C3_KIND_PILEUP) == 5);
    setenv("C3HIP_OCCLUDE_CHUNK", "-3", 1);
    CHECK(occlude_chunk_env(C3_KIND_FULL_ALIGNMENT) == 64 && occlude_chunk_env(C3_KIND_PILEUP) == 256);
    unsetenv("C3HIP_OCCLUDE_CHUNK");
    const int P = 33;
    // full alignment: depth 89 / C = 8 (the cell form), depth 89 / C = 9 (297-byte rows), depth 55 / C = 18 (even, and not the cell form);
    // counts 0 and 1 at the ends of the passes of every cut
    const struct { int depth, C, row_floats; } shapes[] = {{89, 8, 90 + kDecodeCols}, {89, 9, 90}, {55, 18, 24}};
    for (const auto &g : shapes) {
        const std::vector<std::vector<int32_t>> calls = {{}, {0}, {1}, {g.depth}, {0, 3, 1, 1, 2, 0, 0, g.depth, 1}, {1, 0, 17, 0, 1, 1, 5}};
        for (const auto &count : calls)
            for (int64_t chunk : {1, 3, 0})
                for (int band : {1, 5, P})
                    for (int what : {1, 2, 3}) one_call(false, g.depth, P, g.C, 1, g.row_floats, count, (what + band) % 2 == 0, chunk, what, band);
    }
    // pileup: C = 18 int8 (594-byte windows: 2-byte aligned) and int32, C = 9 and 8 for the walk
    const struct { int C, item, row_floats; } pshapes[] = {{18, 1, 24}, {18, 4, 90 + kDecodeCols}, {9, 1, 90}, {8, 4, 24}};
    for (const auto &g : pshapes)
        for (size_t batch : {0, 1, 4, 7})
            for (int64_t chunk : {1, 3, 0})
                for (int band : {1, 5, P})
                    for (int what : {1, 2, 3}) one_call(true, 1, P, g.C, g.item, g.row_floats, std::vector<int32_t>(batch, 1), false, chunk, what, band);
    c3_model *pileup = new c3_model(), *fa = new c3_model();
    pileup->kind = C3_KIND_PILEUP, pileup->C = 18, pileup->nb = 2, pileup->nout = 24, pileup->row = 24;
    fa->kind = C3_KIND_FULL_ALIGNMENT, fa->C = 9, fa->depth = 55, fa->nb = 4, fa->nout = 90, fa->row = 90 + kDecodeCols;
    entries(pileup, fa);
    delete pileup;
    delete fa;
    printf("occlude_host_check: %d failure(s)\n", failures);
    return failures != 0;
}
