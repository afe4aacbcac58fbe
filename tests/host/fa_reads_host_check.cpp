// fa_reads_host_check.cpp -- the host form of full alignment from reads (clair3_amd/csrc/c3_fa_rule.h: the checks, the tables, the rule, the
// alt-info text) as a stand-alone program with its own main, so that it can run under AddressSanitizer and UndefinedBehaviorSanitizer on a
// CPU.  Plain C++: no HIP, no device, no library.  tests/test_fa_reads.py builds and drives it:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/fa_reads_host_check.cpp -o fa_reads_host_check
//   fa_reads_host_check CASE.bin OUT.bin   replays one read set.  CASE.bin: twelve int64 (n_reads, n_ops, seq_bytes, qual_bytes, n_cand,
//       ref_first, ref_len, min_mq, max_indel_length, matrix_depth, seed, with_names), then pos, flag, mapq, cigar_first, cigar, seq_first,
//       seq, qual_first, qual, haplotype, name_key, centres, ref as raw arrays.  OUT.bin: n_rows, text bytes (int64), rows, counts, depths, text
//   fa_reads_host_check --errors           the refused inputs: each must fail with a message (and the N op with its own code), none may crash
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
#include "../../clair3_amd/csrc/c3_fa_rule.h"

template <typename T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run(const c3_read_set &rs, const c3_read_extras &ex, const int64_t *centres, int64_t n_cand, const uint8_t *ref, int64_t ref_first,
               int64_t ref_len, const c3_fa_config &cfg, c3::FaResult &out) {
    c3::FaTables t;
    const int rc = c3::fa_check(&rs, &ex, centres, n_cand, ref, ref_first, ref_len, &cfg, t);
    if (rc) return rc;
    out.clear();
    if (n_cand == 0) return 0;
    const c3::FaView v = c3::fa_view(&rs, &ex, t, ref, ref_first);
    int64_t deep = 0;
    c3::fa_rule_host(&rs, t, v, centres, n_cand, cfg, out, &deep);
    return 0;
}

static int errors() {
    // two reads: 30M at 100, and 10M 5N 15M at 104
    const int64_t pos[2] = {100, 104}, unsorted[2] = {104, 100}, cf[3] = {0, 1, 4}, sf[3] = {0, 15, 28}, qf[3] = {0, 30, 55};
    const uint16_t flag[2] = {0, 16};
    const uint8_t mapq[2] = {60, 60}, hap[2] = {1, 2}, bad_hap[2] = {1, 3};
    std::vector<uint8_t> seq(28, 0x12), qual(55, 30), ref(400, 'A');
    const uint32_t cigar[4] = {30u << 4, 10u << 4, 5u << 4 | 3, 15u << 4}, no_skip[4] = {30u << 4, 10u << 4, 5u << 4 | 2, 15u << 4};
    const int64_t centres[2] = {110, 140}, low[1] = {15}, descending[2] = {140, 110}, twice[2] = {110, 110}, far[1] = {300};
    c3_fa_config cfg{};
    cfg.min_mq = 5, cfg.max_indel_length = 50, cfg.matrix_depth = 89;
    c3::FaResult out;
    int bad = 0;
    auto expect = [&](const char *what, int rc, int want) {
        const bool ok = rc == want && (want == 0 || !g_err.empty());
        printf("%-36s %s%s%s\n", what, ok ? "ok" : "WRONG", want ? ": " : "", want ? g_err.c_str() : "");
        bad += !ok, g_err.clear();
    };
    c3_read_set rs{2, pos, flag, mapq, cf, no_skip, sf, seq.data()};
    c3_read_extras ex{qf, qual.data(), hap, nullptr};
    expect("a good read set", run(rs, ex, centres, 2, ref.data(), 0, 400, cfg, out), 0);
    if (out.count.size() != 2 || out.count[0] != 2) return printf("WRONG: %zu candidates\n", out.count.size()), 1;
    expect("no candidates", run(rs, ex, nullptr, 0, ref.data(), 0, 400, cfg, out), 0);
    c3_read_set a = rs;
    a.cigar = cigar;
    expect("an N op over a window", run(a, ex, centres, 2, ref.data(), 0, 400, cfg, out), C3_FA_ERR_REFSKIP);
    expect("an N op outside every window", run(a, ex, far, 1, ref.data(), 0, 400, cfg, out), 0);
    a = rs, a.pos = unsorted;
    expect("unsorted reads", run(a, ex, centres, 2, ref.data(), 0, 400, cfg, out), 1);
    expect("a candidate below 16", run(rs, ex, low, 1, ref.data(), 0, 400, cfg, out), 1);
    expect("candidates descending", run(rs, ex, descending, 2, ref.data(), 0, 400, cfg, out), 1);
    expect("a candidate twice", run(rs, ex, twice, 2, ref.data(), 0, 400, cfg, out), 1);
    expect("reference too short", run(rs, ex, centres, 2, ref.data(), 0, 206, cfg, out), 1);
    expect("reference starts late", run(rs, ex, centres, 2, ref.data(), 95, 305, cfg, out), 1);
    c3_read_extras b = ex;
    b.haplotype = bad_hap;
    expect("haplotype 3", run(rs, b, centres, 2, ref.data(), 0, 400, cfg, out), 1);
    const int64_t short_q[3] = {0, 29, 54};
    b = ex, b.qual_first = short_q;
    expect("qual shorter than the query", run(rs, b, centres, 2, ref.data(), 0, 400, cfg, out), 1);
    c3_fa_config c2 = cfg;
    c2.matrix_depth = 0;
    expect("matrix_depth 0", run(rs, ex, centres, 2, ref.data(), 0, 400, c2, out), 1);
    c3_read_set none{};
    expect("an empty read set", run(none, ex, centres, 2, ref.data(), 0, 400, cfg, out), 0);
    if (out.count.size() != 2 || out.count[0] != 0 || !out.rows.empty()) return printf("WRONG: the empty read set has rows\n"), 1;
    return bad != 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "--errors") return errors();
    if (argc != 3) return fprintf(stderr, "usage: %s CASE.bin OUT.bin | --errors\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    int64_t h[12];
    if (!f || fread(h, 8, 12, f) != 12) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    const size_t n = (size_t)h[0];
    std::vector<int64_t> pos, cigar_first, seq_first, qual_first, centres;
    std::vector<uint16_t> flag;
    std::vector<uint8_t> mapq, seq, qual, hap, ref;
    std::vector<uint32_t> cigar;
    std::vector<uint64_t> names;
    const bool ok = get(f, pos, n) && get(f, flag, n) && get(f, mapq, n) && get(f, cigar_first, n + 1) && get(f, cigar, (size_t)h[1]) &&
                    get(f, seq_first, n + 1) && get(f, seq, (size_t)h[2]) && get(f, qual_first, n + 1) && get(f, qual, (size_t)h[3]) && get(f, hap, n) &&
                    get(f, names, n) && get(f, centres, (size_t)h[4]) && get(f, ref, (size_t)h[6]);
    fclose(f);
    if (!ok) return fprintf(stderr, "%s is short\n", argv[1]), 2;
    const c3_read_set rs{h[0], pos.data(), flag.data(), mapq.data(), cigar_first.data(), cigar.data(), seq_first.data(), seq.data()};
    const c3_read_extras ex{qual_first.data(), qual.data(), hap.data(), h[11] ? names.data() : nullptr};
    c3_fa_config cfg{};
    cfg.min_mq = (int32_t)h[7], cfg.max_indel_length = (int32_t)h[8], cfg.matrix_depth = (int32_t)h[9], cfg.seed = (uint64_t)h[10];
    c3::FaResult out;
    if (run(rs, ex, centres.data(), h[4], ref.data(), h[5], h[6], cfg, out)) return fprintf(stderr, "refused: %s\n", g_err.c_str()), 1;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    const int64_t sizes[2] = {(int64_t)(out.rows.size() / c3::kFaRowBytes), (int64_t)out.text.size()};
    fwrite(sizes, 8, 2, o);
    fwrite(out.rows.data(), 1, out.rows.size(), o), fwrite(out.count.data(), 4, out.count.size(), o), fwrite(out.depth.data(), 4, out.depth.size(), o);
    fwrite(out.text.data(), 1, out.text.size(), o);
    fclose(o);
    return 0;
}
