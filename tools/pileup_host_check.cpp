// pileup_host_check.cpp -- the host form of pileup from reads (csrc/c3_pileup_rule.h: the checks, the rule, the alt-info printer) as a
// stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU.  tools/pileup_host_check.py builds and drives it.
//
//   pileup_host_check CASE.bin OUT.bin [max_indel_length call_ht]   replays one read set: CASE.bin holds seven int64 (n_reads, n_ops,
//       seq_bytes, start, end, ref_first, ref_len) and then pos, flag, mapq, cigar_first, cigar, seq_first, seq, ref as raw arrays; OUT.bin
//       gets n_cols, n_cand (int64), the matrix, major, and the text
//   pileup_host_check --errors                                      the refused inputs: each must fail with a message, none may crash
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../include/c3hip.h"

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
#include "../clair3_amd/csrc/c3_pileup_rule.h"

struct Case {
    int64_t h[7];
    std::vector<int64_t> pos, cigar_first, seq_first;
    std::vector<uint16_t> flag;
    std::vector<uint8_t> mapq, seq, ref;
    std::vector<uint32_t> cigar;
    c3_read_set rs() const { return c3_read_set{h[0], pos.data(), flag.data(), mapq.data(), cigar_first.data(), cigar.data(), seq_first.data(), seq.data()}; }
};
template <typename T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static c3_pileup_config config(int max_indel, int call_ht) {
    c3_pileup_config c{};
    c.min_mq = 5, c.max_indel_length = max_indel, c.gvcf = 1, c.call_ht = call_ht, c.hash_mask = ~0ull;
    return c;
}
static int run(const c3_read_set &rs, int64_t start, int64_t end, const uint8_t *ref, int64_t ref_first, int64_t ref_len, const c3_pileup_config &cfg,
               c3::PileupResult &out) {
    c3::PileupCensus census;
    if (c3::pileup_check(&rs, start, end, ref, ref_first, ref_len, &cfg, &census)) return 1;
    int64_t events = 0;
    c3::pileup_rule_host(&rs, start, end, ref, ref_first, cfg, out, &events);
    return 0;
}

static int errors() {
    const int64_t pos[2] = {10, 12}, cf[3] = {0, 1, 4}, sf[3] = {0, 5, 10}, cf_bad[3] = {0, 3, 2};
    const uint16_t flag[2] = {0, 16};
    const uint8_t mapq[2] = {60, 60}, seq[10] = {0x12, 0x48, 0x12, 0x48, 0x12, 0x48, 0x12, 0x48, 0x12, 0x48};
    const uint32_t cigar[4] = {10u << 4, 4u << 4, 2u << 4 | 1, 4u << 4}, overrun[4] = {10u << 4, 4u << 4, 3u << 4 | 1, 4u << 4};
    const uint32_t zero_len[4] = {10u << 4, 4u << 4, 0u << 4 | 1, 6u << 4}, bad_op[4] = {10u << 4, 4u << 4, 2u << 4 | 9, 4u << 4};
    std::vector<uint8_t> ref(200, 'A');
    c3::PileupResult out;
    const c3_pileup_config cfg = config(50, 0);
    int bad = 0;
    auto expect = [&](const char *what, int rc, bool want_fail) {
        const bool ok = (rc != 0) == want_fail && (!want_fail || !g_err.empty());
        printf("%-28s %s%s%s\n", what, ok ? "ok" : "WRONG", want_fail ? ": " : "", want_fail ? g_err.c_str() : "");
        bad += !ok, g_err.clear();
    };
    c3_read_set rs{2, pos, flag, mapq, cf, cigar, sf, seq};
    expect("a good read set", run(rs, 5, 40, ref.data(), 0, 200, cfg, out), false);
    if (out.major.size() != 10) return printf("WRONG: %zu columns\n", out.major.size()), 1;
    expect("reference too short", run(rs, 5, 40, ref.data(), 0, 60, cfg, out), true);
    expect("reference starts late", run(rs, 5, 40, ref.data(), 6, 194, cfg, out), true);
    expect("end <= start", run(rs, 40, 40, ref.data(), 0, 200, cfg, out), true);
    c3_read_set a = rs;
    a.cigar_first = cf_bad;
    expect("cigar_first decreasing", run(a, 5, 40, ref.data(), 0, 200, cfg, out), true);
    a = rs, a.cigar = overrun;
    expect("CIGAR overruns its seq", run(a, 5, 40, ref.data(), 0, 200, cfg, out), true);
    a = rs, a.cigar = zero_len;
    expect("op of length 0", run(a, 5, 40, ref.data(), 0, 200, cfg, out), true);
    a = rs, a.cigar = bad_op;
    expect("op code 9", run(a, 5, 40, ref.data(), 0, 200, cfg, out), true);
    a = rs, a.pos = nullptr;
    expect("null pos", run(a, 5, 40, ref.data(), 0, 200, cfg, out), true);
    c3_read_set none{};
    expect("an empty read set", run(none, 5, 40, ref.data(), 0, 200, cfg, out), false);
    if (!out.major.empty() || out.n_ref.size() != 35) return printf("WRONG: the empty read set has columns\n"), 1;
    return bad != 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "--errors") return errors();
    if (argc != 3 && argc != 5) return fprintf(stderr, "usage: %s CASE.bin OUT.bin [max_indel_length call_ht] | --errors\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    Case c;
    if (!f || fread(c.h, 8, 7, f) != 7) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    const size_t n = (size_t)c.h[0];
    const bool ok = get(f, c.pos, n) && get(f, c.flag, n) && get(f, c.mapq, n) && get(f, c.cigar_first, n + 1) && get(f, c.cigar, (size_t)c.h[1]) &&
                    get(f, c.seq_first, n + 1) && get(f, c.seq, (size_t)c.h[2]) && get(f, c.ref, (size_t)c.h[6]);
    fclose(f);
    if (!ok) return fprintf(stderr, "%s is short\n", argv[1]), 2;
    c3::PileupResult out;
    const c3_pileup_config cfg = argc == 5 ? config(atoi(argv[3]), atoi(argv[4])) : config(50, 0);
    if (run(c.rs(), c.h[3], c.h[4], c.ref.data(), c.h[5], c.h[6], cfg, out)) return fprintf(stderr, "refused: %s\n", g_err.c_str()), 1;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    const int64_t sizes[2] = {(int64_t)out.major.size(), (int64_t)out.cand_pos.size()};
    fwrite(sizes, 8, 2, o);
    fwrite(out.matrix.data(), 4, out.matrix.size(), o), fwrite(out.major.data(), 8, out.major.size(), o);
    fwrite(out.text.data(), 1, out.text.size(), o);
    fclose(o);
    return 0;
}
