// haplotag_host_check.cpp -- the host form of haplotagging the reads (clair3_amd/csrc/c3_hap_rule.h: the checks, the tables, the rule) as a
// stand-alone program with its own main, so that it can run under AddressSanitizer and UndefinedBehaviorSanitizer on a CPU.  Plain C++: no
// HIP, no device, no library.  tests/test_haplotag.py builds and drives it:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/haplotag_host_check.cpp -o haplotag_host_check
//   haplotag_host_check CASE.bin OUT.bin   replays one read set.  CASE.bin: seven int64 (n_reads, n_ops, seq_bytes, n_variants, ref_first,
//       ref_len, min_haplotag_mq), then pos, mapq, cigar_first, cigar, seq_first, seq, the variants' pos, alt_base, genotype, phase_set and
//       ref as raw arrays.  OUT.bin: n_reads, n_pairs (int64), hap, alleles, pair_first
//   haplotag_host_check --errors           the refused inputs: each must fail with a message, none may crash
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
#include "../../clair3_amd/csrc/c3_hap_rule.h"

template <typename T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run(const c3_read_set &rs, const c3_phased_variants &vs, const uint8_t *ref, int64_t ref_first, int64_t ref_len, const c3_haplotag_config &cfg,
               c3::HapResult &out) {
    c3::HapTables t;
    const int rc = c3::hap_check(&rs, &vs, ref, ref_first, ref_len, &cfg, t);
    if (rc) return rc;
    c3::hap_rule_host(c3::hap_view(&rs, &vs, t, ref, ref_first), out);
    return 0;
}

static int errors() {
    // two reads: 30M at 100, and 10M 5N 15M at 104; two variants under them
    const int64_t pos[2] = {100, 104}, cf[3] = {0, 1, 4}, sf[3] = {0, 15, 28};
    const uint16_t flag[2] = {0, 16};
    const uint8_t mapq[2] = {60, 60};
    std::vector<uint8_t> seq(28, 0x12), ref(400, 'A');
    const uint32_t cigar[4] = {30u << 4, 10u << 4, 5u << 4 | 3, 15u << 4}, zero_len[4] = {30u << 4, 10u << 4, 0u << 4 | 2, 15u << 4};
    const int64_t vpos[2] = {110, 120}, descending[2] = {120, 110}, twice[2] = {110, 110};
    const uint8_t alt[2] = {'C', 'G'}, gt[2] = {1, 2}, bad_gt[2] = {1, 3}, zero_gt[2] = {0, 1};
    const int32_t ps[2] = {7, 7};
    c3_haplotag_config cfg{};
    cfg.min_haplotag_mq = 20;
    c3::HapResult out;
    int bad = 0;
    auto expect = [&](const char *what, int rc, int want) {
        const bool ok = rc == want && (want == 0 || !g_err.empty());
        printf("%-36s %s%s%s\n", what, ok ? "ok" : "WRONG", want ? ": " : "", want ? g_err.c_str() : "");
        bad += !ok, g_err.clear();
    };
    const c3_read_set rs{2, pos, flag, mapq, cf, cigar, sf, seq.data()};
    const c3_phased_variants vs{2, vpos, alt, gt, ps};
    expect("a good read set", run(rs, vs, ref.data(), 0, 400, cfg, out), 0);
    if (out.hap.size() != 2 || out.pair_first.size() != 3 || out.pair_first[2] != 4) return printf("WRONG: %zu reads\n", out.hap.size()), 1;
    c3_phased_variants v = vs;
    v.n = 0;
    expect("no variants", run(rs, v, ref.data(), 0, 400, cfg, out), 0);
    if (out.hap[0] != 0 || out.hap[1] != 0 || !out.alleles.empty()) return printf("WRONG: tags without variants\n"), 1;
    v = vs, v.pos = nullptr;
    expect("null positions", run(rs, v, ref.data(), 0, 400, cfg, out), 1);
    v = vs, v.phase_set = nullptr;
    expect("null phase sets", run(rs, v, ref.data(), 0, 400, cfg, out), 1);
    v = vs, v.pos = descending;
    expect("variants descending", run(rs, v, ref.data(), 0, 400, cfg, out), 1);
    v = vs, v.pos = twice;
    expect("a variant twice", run(rs, v, ref.data(), 0, 400, cfg, out), 1);
    v = vs, v.genotype = bad_gt;
    expect("genotype 3", run(rs, v, ref.data(), 0, 400, cfg, out), 1);
    v = vs, v.genotype = zero_gt;
    expect("genotype 0", run(rs, v, ref.data(), 0, 400, cfg, out), 1);
    expect("reference too short", run(rs, vs, ref.data(), 0, 130, cfg, out), 1);
    expect("reference just long enough", run(rs, vs, ref.data(), 0, 131, cfg, out), 0);
    expect("reference starts late", run(rs, vs, ref.data() + 101, 101, 299, cfg, out), 1);
    expect("reference starts just in time", run(rs, vs, ref.data() + 100, 100, 300, cfg, out), 0);
    expect("null reference", run(rs, vs, nullptr, 0, 400, cfg, out), 1);
    c3_haplotag_config high = cfg;
    high.min_haplotag_mq = 61;
    expect("no read is tagged: no reference needed", run(rs, vs, nullptr, 0, 0, high, out), 0);
    c3_read_set a = rs;
    a.cigar = zero_len;
    expect("a CIGAR op of length 0", run(a, vs, ref.data(), 0, 400, cfg, out), 1);
    a = rs, a.mapq = nullptr;
    expect("null mapq", run(a, vs, ref.data(), 0, 400, cfg, out), 1);
    const int64_t short_s[3] = {0, 14, 27};
    a = rs, a.seq_first = short_s;
    expect("seq shorter than the query", run(a, vs, ref.data(), 0, 400, cfg, out), 1);
    c3_haplotag_config neg = cfg;
    neg.min_haplotag_mq = -1;
    expect("a negative min_haplotag_mq", run(rs, vs, ref.data(), 0, 400, neg, out), 1);
    c3_read_set none{};
    expect("an empty read set", run(none, vs, ref.data(), 0, 400, cfg, out), 0);
    if (!out.hap.empty() || out.pair_first.size() != 1) return printf("WRONG: the empty read set has tags\n"), 1;
    return bad != 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "--errors") return errors();
    if (argc != 3) return fprintf(stderr, "usage: %s CASE.bin OUT.bin | --errors\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    int64_t h[7];
    if (!f || fread(h, 8, 7, f) != 7) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    const size_t n = (size_t)h[0], nv = (size_t)h[3];
    std::vector<int64_t> pos, cigar_first, seq_first, vpos;
    std::vector<uint8_t> mapq, seq, valt, vgt, ref;
    std::vector<uint32_t> cigar;
    std::vector<int32_t> vps;
    const bool ok = get(f, pos, n) && get(f, mapq, n) && get(f, cigar_first, n + 1) && get(f, cigar, (size_t)h[1]) && get(f, seq_first, n + 1) &&
                    get(f, seq, (size_t)h[2]) && get(f, vpos, nv) && get(f, valt, nv) && get(f, vgt, nv) && get(f, vps, nv) && get(f, ref, (size_t)h[5]);
    fclose(f);
    if (!ok) return fprintf(stderr, "%s is short\n", argv[1]), 2;
    const c3_read_set rs{h[0], pos.data(), nullptr, mapq.data(), cigar_first.data(), cigar.data(), seq_first.data(), seq.data()};
    const c3_phased_variants vs{h[3], vpos.data(), valt.data(), vgt.data(), vps.data()};
    c3_haplotag_config cfg{};
    cfg.min_haplotag_mq = (int32_t)h[6];
    c3::HapResult out;
    if (run(rs, vs, ref.data(), h[4], h[5], cfg, out)) return fprintf(stderr, "refused: %s\n", g_err.c_str()), 1;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
    const int64_t sizes[2] = {(int64_t)out.hap.size(), (int64_t)out.alleles.size()};
    fwrite(sizes, 8, 2, o);
    fwrite(out.hap.data(), 1, out.hap.size(), o), fwrite(out.alleles.data(), 1, out.alleles.size(), o);
    fwrite(out.pair_first.data(), 8, out.pair_first.size(), o);
    fclose(o);
    return 0;
}
