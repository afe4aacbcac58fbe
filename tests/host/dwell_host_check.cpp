// dwell_host_check.cpp -- the host form of the dwell channel (clair3_amd/csrc/c3_dwell_rule.h with c3_fa_rule.h: the checks, the per-read
// tables, the 9-channel rows) as a stand-alone program with its own main, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer on a CPU.  Plain C++: no HIP, no device, no library.  tests/test_dwell.py builds and drives it:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/dwell_host_check.cpp -o dwell_host_check
//   dwell_host_check CASE.bin OUT.bin   replays one read set.  CASE.bin: thirteen int64 (n_reads, n_ops, seq_bytes, qual_bytes, n_cand,
//       ref_first, ref_len, min_mq, max_indel_length, matrix_depth, seed, with_names, n_moves), then pos, flag, mapq, cigar_first, cigar,
//       seq_first, seq, qual_first, qual, haplotype, name_key, centres, ref, mv_first, mv as raw arrays, each in a heap block of exactly its
//       size: the last read's table ends at the end of the staged array.  OUT.bin: n_rows, n_cum (int64), rows (297 bytes each), cum
//   dwell_host_check --tables           tables by hand, each in a heap block of exactly its size, and the refused inputs
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../include/c3hip.h"

static std::string g_err;
static int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}
#include "../../clair3_amd/csrc/c3_dwell_rule.h"

template <typename T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    v.shrink_to_fit();
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int tables() {
    int bad = 0;
    auto expect = [&](const char *what, std::vector<int8_t> mv, int64_t l, bool reverse, bool has, std::vector<int32_t> want) {
        mv.shrink_to_fit();
        std::vector<int32_t> cum((size_t)l + 1, -1);
        cum.shrink_to_fit();
        const bool got = c3::fa_dwell_cum_host(mv.empty() ? nullptr : mv.data(), (int64_t)mv.size(), l, reverse, cum.data());
        const bool ok = got == has && cum == want;
        printf("%-44s %s\n", what, ok ? "ok" : "WRONG");
        bad += !ok;
    };
    expect("no tag", {}, 3, false, false, {0, 0, 0, 0});
    expect("the stride alone", {5}, 3, false, false, {0, 0, 0, 0});
    expect("no query bases", {5, 1, 0, 1}, 0, false, false, {0});
    expect("no move behind the stride", {5, 0, 0, 0}, 2, false, true, {0, 0, 0});
    expect("zeros in front belong to nobody", {5, 0, 0, 1, 0, 1, 0, 0}, 2, false, true, {0, 2, 5});
    expect("the same, reversed", {5, 0, 0, 1, 0, 1, 0, 0}, 2, true, true, {0, 3, 5});
    expect("K < l: zeros behind", {0, 1, 0, -1}, 4, false, true, {0, 2, 3, 3, 3});
    expect("K < l, reversed", {0, 1, 0, -1}, 4, true, true, {0, 0, 0, 1, 3});
    expect("K > l: the bases behind l are dropped", {5, 1, 1, 0, 1, 0, 0, 1}, 2, false, true, {0, 1, 3});
    expect("a move on the last entry", {5, 1, 0, 0, 7}, 2, false, true, {0, 3, 4});
    // the refused inputs of a c3_read_moves
    c3::FaTables t;
    t.qfirst = {0, 4, 8};
    c3::DwTables d;
    const int64_t good[3] = {0, 5, 9}, down[3] = {0, 5, 4}, negative[3] = {-1, 5, 9};
    const int8_t mv[9] = {5, 1, 0, 1, 1, 5, 1, 1, 1};
    auto refused = [&](const char *what, const c3_read_moves *m, int want) {
        g_err.clear();
        const int rc = c3::fa_dwell_check(m, t, 2, d, "check");
        const bool ok = rc == want && (want == 0) == g_err.empty();
        printf("%-44s %s%s%s\n", what, ok ? "ok" : "WRONG", want ? ": " : "", g_err.c_str());
        bad += !ok;
    };
    c3_read_moves m{good, mv};
    refused("good offsets", &m, 0);
    refused("null moves", nullptr, 1);
    m.mv_first = down;
    refused("decreasing offsets", &m, 1);
    m.mv_first = negative;
    refused("a negative offset", &m, 1);
    m.mv_first = good, m.mv = nullptr;
    refused("null mv", &m, 1);
    m.mv_first = nullptr;
    refused("null mv_first", &m, 1);
    return bad != 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "--tables") return tables();
    if (argc != 3) return fprintf(stderr, "usage: %s CASE.bin OUT.bin | --tables\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    int64_t h[13];
    if (!f || fread(h, 8, 13, f) != 13) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    const size_t n = (size_t)h[0];
    std::vector<int64_t> pos, cigar_first, seq_first, qual_first, centres, mv_first;
    std::vector<uint16_t> flag;
    std::vector<uint8_t> mapq, seq, qual, hap, ref;
    std::vector<uint32_t> cigar;
    std::vector<uint64_t> names;
    std::vector<int8_t> mv;
    const bool ok = get(f, pos, n) && get(f, flag, n) && get(f, mapq, n) && get(f, cigar_first, n + 1) && get(f, cigar, (size_t)h[1]) &&
                    get(f, seq_first, n + 1) && get(f, seq, (size_t)h[2]) && get(f, qual_first, n + 1) && get(f, qual, (size_t)h[3]) && get(f, hap, n) &&
                    get(f, names, n) && get(f, centres, (size_t)h[4]) && get(f, ref, (size_t)h[6]) && get(f, mv_first, n + 1) && get(f, mv, (size_t)h[12]);
    fclose(f);
    if (!ok) return fprintf(stderr, "%s is short\n", argv[1]), 2;
    const c3_read_set rs{h[0], pos.data(), flag.data(), mapq.data(), cigar_first.data(), cigar.data(), seq_first.data(), seq.data()};
    const c3_read_extras ex{qual_first.data(), qual.data(), hap.data(), h[11] ? names.data() : nullptr};
    const c3_read_moves moves{mv_first.data(), mv.data()};
    c3_fa_config cfg{};
    cfg.min_mq = (int32_t)h[7], cfg.max_indel_length = (int32_t)h[8], cfg.matrix_depth = (int32_t)h[9], cfg.seed = (uint64_t)h[10];
    c3::FaTables t;
    c3::DwTables d;
    if (c3::fa_check(&rs, &ex, centres.data(), h[4], ref.data(), h[5], h[6], &cfg, t) || c3::fa_dwell_check(&moves, t, h[0], d, "dwell_host_check"))
        return fprintf(stderr, "refused: %s\n", g_err.c_str()), 1;
    std::vector<int32_t> cum;
    c3::fa_dwell_tables_host(&rs, &moves, t, d, cum);
    cum.shrink_to_fit();
    c3::FaResult out;
    int64_t deep = 0;
    if (h[4] > 0) c3::fa_rule_host(&rs, t, c3::fa_view(&rs, &ex, t, ref.data(), h[5]), centres.data(), h[4], cfg, out, &deep, cum.data());
    FILE *o = fopen(argv[2], "wb");
    if (!o) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    const int64_t sizes[2] = {(int64_t)(out.rows.size() / c3::kDwRowBytes), (int64_t)cum.size()};
    fwrite(sizes, 8, 2, o);
    fwrite(out.rows.data(), 1, out.rows.size(), o), fwrite(cum.data(), 4, cum.size(), o);
    fclose(o);
    return 0;
}
