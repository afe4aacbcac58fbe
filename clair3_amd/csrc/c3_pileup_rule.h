// c3_pileup_rule.h -- pileup from reads, the rule: what calculate_clair3_pileup (src/clair3_pileup.c:208-461) makes of the columns htslib
// hands it, restated over aligned reads as the arrays a BAM record holds (c3_read_set, include/c3hip.h).  Plain host C++: no HIP, no
// library; it compiles into a stand-alone program as it is (tools/pileup_host_check.cpp).  The including file provides fail().
// pileup_site() is the one statement of the per-column arithmetic: the host form below and the kernels of c3_pileup.h both call it.
//
// READ FILTER (src/medaka_bamiter.c:20-22): a read with one of the flags 0x4 | 0x100 | 0x800 | 0x200 | 0x400, or with mapq < min_mq, is
// dropped.  The tag and read-group filters of read_bam are not restated.
// COLUMNS: a column exists for every position of [start, end) that a kept read spans with an M, =, X, D or N op; major lists them in
// increasing order (:208, :220-222, :240).
// PER READ AT p: N: nothing is counted, nothing is added to depth (:250 is_refskip).  D: channel 8 / 17 by strand, depth + 1 (:275-278).
// M, =, X: nt16 codes 1, 2, 4, 8 count in channels 0 .. 3, or 9 .. 12 on the reverse strand, depth + 1 (:281-286).
//   DEVIATION: for every other code the reference indexes num2countbaseclair3[...] = -1 and adds into the LAST channel of the column in
//   front (:283-286).  That is a defect and is not reproduced: such a base adds to depth and counts in no channel.
// INDEL AT p (:252-271, :290-304: p->indel of the column p): p is the last reference position of an M, =, X or D op; of the ops behind it,
// P skipped, the first decides: an I is an insertion whose string is the bases of that I and of every I directly behind it; a D is a
// deletion of its length, attributed to p.  An indel in front of the read's first spanned position is thereby dropped, and so is one
// behind an N.  An event whose p lies outside [start, end) is dropped; its deleted bases inside the region still count.
//   These adjacency rules restate htslib's column resolution (resolve_cigar2) from its documented behaviour.  They were NOT checked
//   against htslib, which is not available where this was written.
// PER COLUMN (:307-371): channels 6 / 15 the deletion starts per strand, 7 / 16 the largest count of one length; 4 / 13 the insertions per
// strand, 5 / 14 the largest count of one string; the reference base's channels then become minus the sum of channels 0 .. 3 and minus the
// sum of 9 .. 12.  The reference base is upper_base of the reference byte; its index is base2index: C 1, G 2, T 3, anything else 0.
// ref_count, alt_count, major_alt_base, all_alt_count: the loop :355-368 as it stands, all_alt_count growing only by a new maximum.
// CANDIDATE (:374-390): depth = max(1, depth); the majority tests, the equal-majority tie on ref_base - major_alt_base < 0, the float32
// ratio tests, call_snp_only, min_depth, reference base in ACGT; unless call_ht, contiguous_flanking_num >= 16: the consecutive existing
// columns directly to the left, reset by a gap and by the reference's pre_pos == 0 (:225-229: the column behind position 0 starts at 0).
// ALT-INFO (:399-447): "<pos + 1>-<depth>-<ref>-", X<b> n for the non-reference bases in ACGT order, D<ref bytes> n per deletion length
// ascending, strands merged, lengths <= max_indel_length; I<ref><string> n per distinct string, strands merged, lengths <=
// max_indel_length, ORDERED BY LENGTH THEN BYTES (the reference's khash order is unspecified; its consumers split the line into a dict);
// R<ref> n when ref_depth = ref_count - all deletions - all insertions > 0 (every length counts there).
// GVCF COUNTS (:452-455): n_ref = ref_count, n_total = ref_count + all_alt_count + del_count + ins_count, at p - start; 0 without a column.
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define C3_PILEUP_HD __host__ __device__ __forceinline__
#else
#define C3_PILEUP_HD inline
#endif

namespace c3 {

constexpr int kPileupChannels = 18;
constexpr int kPileupFlank = 16;               // pileup_flanking_base_num
constexpr uint32_t kPileupDropFlags = 0x4 | 0x100 | 0x800 | 0x200 | 0x400;
constexpr int64_t kPileupMaxSites = (int64_t)1 << 27;
constexpr int64_t kPileupMaxIndelOps = (int64_t)1 << 29;  // I and D ops of the kept reads: the device's event table has twice as many slots, below 2^31
enum : int { kOpM = 0, kOpI = 1, kOpD = 2, kOpN = 3, kOpS = 4, kOpH = 5, kOpP = 6, kOpEq = 7, kOpX = 8 };

C3_PILEUP_HD bool pileup_op_base(int op) { return op == kOpM || op == kOpEq || op == kOpX; }
C3_PILEUP_HD bool pileup_op_ref(int op) { return pileup_op_base(op) || op == kOpD || op == kOpN; }  // consumes the reference
C3_PILEUP_HD bool pileup_op_query(int op) { return pileup_op_base(op) || op == kOpI || op == kOpS; }  // consumes the query
C3_PILEUP_HD bool pileup_op_anchor(int op) { return pileup_op_base(op) || op == kOpD; }  // an indel may follow it
C3_PILEUP_HD int pileup_code(const uint8_t *seq, int64_t first, int64_t q) { return (seq[first + (q >> 1)] >> ((~q & 1) << 2)) & 15; }
// channel of an nt16 code on the forward strand, -1: none
C3_PILEUP_HD int pileup_channel(int code) { return code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : -1; }
C3_PILEUP_HD bool pileup_kept(uint32_t flag, uint32_t mapq, int32_t min_mq) { return !(flag & kPileupDropFlags) && (int32_t)mapq >= min_mq; }

// one column's arithmetic (:347-390, :452-455) from its 18 counts BEFORE the reference base's channels are negated
struct PileupSite {
    int32_t depth;  // max(1, depth)
    int32_t ref_count, alt_count, all_alt, del_count, ins_count, fwd_sum, rev_sum;
    int32_t r;      // base2index of the reference base
    uint8_t ref_base, major_alt;
    bool pass;      // pass_af without the flanking test
};
C3_PILEUP_HD PileupSite pileup_site(const int32_t *m, int32_t raw_depth, uint8_t ref_raw, const c3_pileup_config &cfg) {
    PileupSite s;
    s.ref_base = (ref_raw >= 'a' && ref_raw <= 'z') ? (uint8_t)(ref_raw - 32) : ref_raw;
    s.r = s.ref_base == 'C' ? 1 : s.ref_base == 'G' ? 2 : s.ref_base == 'T' ? 3 : 0;
    s.del_count = m[6] + m[15], s.ins_count = m[4] + m[13];
    s.ref_count = s.alt_count = s.all_alt = s.fwd_sum = s.rev_sum = 0, s.major_alt = 0;
    for (int i = 0; i < 4; ++i) {
        s.fwd_sum += m[i], s.rev_sum += m[9 + i];
        const int32_t c = m[i] + m[9 + i];
        if (i == s.r) s.ref_count = c;
        else if (c > s.alt_count) s.alt_count = c, s.major_alt = (uint8_t)"ACGT"[i], s.all_alt += c;
    }
    s.depth = raw_depth > 1 ? raw_depth : 1;
    const float d = (float)s.depth;
#if defined(__HIP_DEVICE_COMPILE__)
    const float snp = __fdiv_rn((float)s.alt_count, d), del = __fdiv_rn((float)s.del_count, d), ins = __fdiv_rn((float)s.ins_count, d);
#else
    const float snp = (float)s.alt_count / d, del = (float)s.del_count / d, ins = (float)s.ins_count / d;
#endif
    const bool acgt = s.ref_base == 'A' || s.ref_base == 'C' || s.ref_base == 'G' || s.ref_base == 'T';
    const bool majority = s.ref_count < s.alt_count || s.ref_count < s.ins_count || s.ref_count < s.del_count;
    const bool tie = s.ref_count > 0 && s.ref_count == s.alt_count && (int)s.ref_base - (int)s.major_alt < 0;
    bool pass;
    if (cfg.call_snp_only) pass = snp >= cfg.min_snp_af;
    else pass = majority || tie || snp >= cfg.min_snp_af || del >= cfg.min_indel_af || ins >= cfg.min_indel_af;
    s.pass = pass && (int64_t)s.depth >= cfg.min_depth && acgt;
    return s;
}
// the raw depth of a column: every channel a read adds to in the walk, and the bases that count in no channel
C3_PILEUP_HD int32_t pileup_raw_depth(const int32_t *m, int32_t other) {
    return m[0] + m[1] + m[2] + m[3] + m[8] + m[9] + m[10] + m[11] + m[12] + m[17] + other;
}

// ------------------------------------------------------------------------------------------ checks shared by both forms
struct PileupCensus {
    int64_t kept = 0, dropped = 0, indel_ops = 0, ops = 0;  // indel_ops: I and D ops of the kept reads
};
static int pileup_check_config(const c3_pileup_config *cfg) {
    if (!cfg) return fail("pileup: null config");
    if (cfg->max_indel_length < 0 || cfg->max_indel_length > (1 << 20)) return fail("pileup: max_indel_length %d outside 0 .. 2^20", cfg->max_indel_length);
    if (cfg->min_depth < 0 || cfg->min_mq < 0) return fail("pileup: a negative min_depth or min_mq");
    if (!(cfg->min_snp_af == cfg->min_snp_af) || !(cfg->min_indel_af == cfg->min_indel_af)) return fail("pileup: a threshold is not a number");
    return 0;
}
// everything a walk relies on: after this no index derived from a CIGAR leaves its read's seq, and every offset fits 32 bits
static int pileup_check(const c3_read_set *rs, int64_t start, int64_t end, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                        const c3_pileup_config *cfg, PileupCensus *census) {
    if (pileup_check_config(cfg)) return 1;
    if (!rs) return fail("pileup: null read set");
    if (start < 0 || end <= start) return fail("pileup: region [%lld, %lld): end <= start or a negative start", (long long)start, (long long)end);
    if (end - start > kPileupMaxSites) return fail("pileup: %lld sites in one call (at most %lld)", (long long)(end - start), (long long)kPileupMaxSites);
    if (!ref_bytes || ref_len < 0 || ref_first < 0 || ref_first > start || ref_first + ref_len <= end + cfg->max_indel_length)
        return fail("pileup: the reference bytes [%lld, %lld) do not cover [%lld, %lld] (region and max_indel_length behind it)", (long long)ref_first,
                    (long long)(ref_first + ref_len), (long long)start, (long long)(end + cfg->max_indel_length));
    const int64_t n = rs->n_reads;
    if (n < 0 || n > INT32_MAX) return fail("pileup: %lld reads", (long long)n);
    if (n > 0 && (!rs->pos || !rs->flag || !rs->mapq || !rs->cigar_first || !rs->seq_first)) return fail("pileup: a null array in the read set");
    if (n == 0) return 0;
    if (rs->cigar_first[0] < 0 || rs->seq_first[0] < 0) return fail("pileup: a negative first offset");
    for (int64_t r = 0; r < n; ++r) {
        if (rs->cigar_first[r + 1] < rs->cigar_first[r]) return fail("pileup: cigar_first is not non-decreasing at read %lld", (long long)r);
        if (rs->seq_first[r + 1] < rs->seq_first[r]) return fail("pileup: seq_first is not non-decreasing at read %lld", (long long)r);
    }
    if (rs->cigar_first[n] > INT32_MAX) return fail("pileup: %lld CIGAR ops in one call", (long long)rs->cigar_first[n]);
    if (rs->cigar_first[n] > rs->cigar_first[0] && !rs->cigar) return fail("pileup: null cigar");
    if (rs->seq_first[n] > rs->seq_first[0] && !rs->seq) return fail("pileup: null seq");
    for (int64_t r = 0; r < n; ++r) {
        if (rs->pos[r] < 0) return fail("pileup: read %lld has a negative position", (long long)r);
        const bool kept = pileup_kept(rs->flag[r], rs->mapq[r], cfg->min_mq);
        int64_t ref = 0, query = 0;
        for (int64_t k = rs->cigar_first[r]; k < rs->cigar_first[r + 1]; ++k) {
            const int op = (int)(rs->cigar[k] & 15);
            const int64_t len = rs->cigar[k] >> 4;
            if (op > kOpX) return fail("pileup: read %lld has the CIGAR op code %d", (long long)r, op);
            if (len == 0) return fail("pileup: read %lld has a CIGAR op of length 0", (long long)r);
            if (pileup_op_ref(op)) ref += len;
            if (pileup_op_query(op)) query += len;
            if (kept && (op == kOpI || op == kOpD)) ++census->indel_ops;
        }
        if (query > 2 * (rs->seq_first[r + 1] - rs->seq_first[r]))
            return fail("pileup: the CIGAR of read %lld consumes %lld bases, its seq holds %lld", (long long)r, (long long)query,
                        (long long)(2 * (rs->seq_first[r + 1] - rs->seq_first[r])));
        if (ref > INT32_MAX || query > INT32_MAX) return fail("pileup: read %lld is longer than 2^31", (long long)r);
        kept ? ++census->kept : ++census->dropped;
    }
    census->ops = rs->cigar_first[n] - rs->cigar_first[0];
    if (census->indel_ops > kPileupMaxIndelOps)
        return fail("pileup: %lld I and D ops in the kept reads (at most %lld a call)", (long long)census->indel_ops, (long long)kPileupMaxIndelOps);
    return 0;
}

// ------------------------------------------------------------------------------------------ the text (host C, both forms)
static const char kNt16[] = "=ACMGRSVTWYHKDBN";  // htslib's seq_nt16_str
struct PileupAllele {  // one entry of a candidate, strands merged
    int32_t len = 0;
    std::string bases;  // insertions: the string; deletions: empty
    int64_t count = 0;
};
static std::string pileup_bases(const c3_read_set *rs, int64_t read, int64_t q, int32_t len) {
    std::string s((size_t)len, '\0');
    for (int32_t i = 0; i < len; ++i) s[(size_t)i] = kNt16[pileup_code(rs->seq, rs->seq_first[read], q + i)];
    return s;
}
static bool pileup_allele_less(const PileupAllele &a, const PileupAllele &b) { return a.len != b.len ? a.len < b.len : a.bases < b.bases; }
// equal neighbours of a sorted list become one entry
static void pileup_merge_sorted(std::vector<PileupAllele> &v) {
    std::sort(v.begin(), v.end(), pileup_allele_less);
    size_t o = 0;
    for (size_t i = 0; i < v.size(); ++i)
        if (o > 0 && v[o - 1].len == v[i].len && v[o - 1].bases == v[i].bases) v[o - 1].count += v[i].count;
        else {
            if (o != i) v[o] = std::move(v[i]);  // (o < i: never onto itself)
            ++o;
        }
    v.resize(o);
}
// one line (:402-446).  x: the four base totals; ref_at: the reference bytes from the candidate's position on
static void pileup_print(std::string &out, int64_t pos, int32_t depth, uint8_t ref_base, int r, const int32_t x[4], const std::vector<PileupAllele> &dels,
                         const std::vector<PileupAllele> &inss, int32_t ref_depth, const uint8_t *ref_at, int32_t max_indel_length) {
    char b[64];
    out.append(b, (size_t)snprintf(b, sizeof(b), "%lld-%d-%c-", (long long)(pos + 1), depth, (char)ref_base));
    for (int i = 0; i < 4; ++i)
        if (x[i] > 0 && i != r) out.append(b, (size_t)snprintf(b, sizeof(b), "X%c %d ", "ACGT"[i], x[i]));
    for (const PileupAllele &d : dels)
        if (d.count > 0 && d.len <= max_indel_length) {
            out.push_back('D');
            out.append((const char *)ref_at + 1, (size_t)d.len);
            out.append(b, (size_t)snprintf(b, sizeof(b), " %lld ", (long long)d.count));
        }
    for (const PileupAllele &a : inss)
        if (a.len <= max_indel_length) {
            out.push_back('I'), out.push_back((char)ref_base);
            out.append(a.bases);
            out.append(b, (size_t)snprintf(b, sizeof(b), " %lld ", (long long)a.count));
        }
    if (ref_depth > 0) out.append(b, (size_t)snprintf(b, sizeof(b), "R%c %d ", (char)ref_base, ref_depth));
    out.push_back('\n');
}

// ------------------------------------------------------------------------------------------ the held result and the host form
struct PileupResult {
    int64_t start = 0, end = 0, n_sites = 0;  // n_sites: of the count pair
    std::vector<int32_t> matrix, cand_depth;
    std::vector<int64_t> major, cand_pos, n_ref, n_total;
    std::string text;
    void clear() { *this = PileupResult(); }
};

struct PileupEvent {  // an insertion or a deletion start of one read
    int64_t col;      // p - start
    int32_t read, q, len;
    uint8_t ins, rev;
};

// the rule, read by read and then column by column.  Checked input only (pileup_check)
static void pileup_rule_host(const c3_read_set *rs, int64_t start, int64_t end, const uint8_t *ref_bytes, int64_t ref_first, const c3_pileup_config &cfg,
                             PileupResult &out, int64_t *n_events) {
    const int64_t n = end - start;
    std::vector<int32_t> img((size_t)n * kPileupChannels, 0), other((size_t)n, 0);
    std::vector<uint8_t> span((size_t)n, 0);
    std::vector<PileupEvent> ev;
    for (int64_t r = 0; r < rs->n_reads; ++r) {
        if (!pileup_kept(rs->flag[r], rs->mapq[r], cfg.min_mq)) continue;
        const int rev = (rs->flag[r] & 16) ? 1 : 0;
        const int64_t c0 = rs->cigar_first[r], c1 = rs->cigar_first[r + 1];
        int64_t rp = rs->pos[r], q = 0;
        for (int64_t k = c0; k < c1; ++k) {
            const int op = (int)(rs->cigar[k] & 15);
            const int64_t len = rs->cigar[k] >> 4;
            const int64_t lo = std::max(rp, start), hi = std::min(rp + len, end);
            if (pileup_op_base(op)) {
                for (int64_t p = lo; p < hi; ++p) {
                    const int ch = pileup_channel(pileup_code(rs->seq, rs->seq_first[r], q + (p - rp)));
                    if (ch >= 0) ++img[(size_t)(p - start) * kPileupChannels + ch + 9 * rev];
                    else ++other[(size_t)(p - start)];
                    span[(size_t)(p - start)] = 1;
                }
            } else if (op == kOpD) {
                for (int64_t p = lo; p < hi; ++p) ++img[(size_t)(p - start) * kPileupChannels + 8 + 9 * rev], span[(size_t)(p - start)] = 1;
            } else if (op == kOpN) {
                for (int64_t p = lo; p < hi; ++p) span[(size_t)(p - start)] = 1;
            }
            if (pileup_op_ref(op)) rp += len;
            if (pileup_op_query(op)) q += len;
            if (!pileup_op_anchor(op)) continue;
            const int64_t p = rp - 1;  // the op's last reference position
            if (p < start || p >= end) continue;
            int64_t j = k + 1;
            while (j < c1 && (int)(rs->cigar[j] & 15) == kOpP) ++j;
            if (j >= c1) continue;
            const int next = (int)(rs->cigar[j] & 15);
            if (next == kOpI) {
                int64_t total = 0;
                for (int64_t i = j; i < c1 && (int)(rs->cigar[i] & 15) == kOpI; ++i) total += rs->cigar[i] >> 4;
                ev.push_back(PileupEvent{p - start, (int32_t)r, (int32_t)q, (int32_t)total, 1, (uint8_t)rev});
            } else if (next == kOpD)
                ev.push_back(PileupEvent{p - start, (int32_t)r, (int32_t)q, (int32_t)(rs->cigar[j] >> 4), 0, (uint8_t)rev});
        }
    }
    *n_events = (int64_t)ev.size();
    // events by column
    std::stable_sort(ev.begin(), ev.end(), [](const PileupEvent &a, const PileupEvent &b) { return a.col < b.col; });
    out.clear();
    out.start = start, out.end = end, out.n_sites = cfg.gvcf ? n : 0;
    out.n_ref.assign((size_t)out.n_sites, 0), out.n_total.assign((size_t)out.n_sites, 0);
    size_t e = 0;
    int64_t pre_pos = 0, flank = 0;
    std::vector<PileupAllele> del[2], ins[2], dels, inss;
    for (int64_t i = 0; i < n; ++i) {
        while (e < ev.size() && ev[e].col < i) ++e;
        int32_t *m = &img[(size_t)i * kPileupChannels];
        const int32_t raw = pileup_raw_depth(m, other[(size_t)i]);
        if (!span[(size_t)i]) continue;
        const int64_t pos = start + i;
        if (pre_pos + 1 != pos || pre_pos == 0) flank = 0;
        else ++flank;
        pre_pos = pos;
        for (int s = 0; s < 2; ++s) del[s].clear(), ins[s].clear();
        for (; e < ev.size() && ev[e].col == i; ++e) {
            PileupAllele a;
            a.len = ev[e].len, a.count = 1;
            if (ev[e].ins) a.bases = pileup_bases(rs, ev[e].read, ev[e].q, ev[e].len);
            (ev[e].ins ? ins : del)[ev[e].rev].push_back(std::move(a));
        }
        for (int s = 0; s < 2; ++s) {
            pileup_merge_sorted(del[s]), pileup_merge_sorted(ins[s]);
            for (const PileupAllele &a : del[s]) m[6 + 9 * s] += (int32_t)a.count, m[7 + 9 * s] = std::max(m[7 + 9 * s], (int32_t)a.count);
            for (const PileupAllele &a : ins[s]) m[4 + 9 * s] += (int32_t)a.count, m[5 + 9 * s] = std::max(m[5 + 9 * s], (int32_t)a.count);
        }
        const uint8_t *ref_at = ref_bytes + (pos - ref_first);
        const PileupSite s = pileup_site(m, raw, *ref_at, cfg);
        const int32_t x[4] = {m[0] + m[9], m[1] + m[10], m[2] + m[11], m[3] + m[12]};
        m[s.r] = -s.fwd_sum, m[9 + s.r] = -s.rev_sum;
        out.matrix.insert(out.matrix.end(), m, m + kPileupChannels);
        out.major.push_back(pos);
        if (cfg.gvcf) out.n_ref[(size_t)i] = s.ref_count, out.n_total[(size_t)i] = (int64_t)s.ref_count + s.all_alt + s.del_count + s.ins_count;
        if (!(s.pass && (cfg.call_ht || flank >= kPileupFlank))) continue;
        dels = del[0], dels.insert(dels.end(), del[1].begin(), del[1].end());
        inss = ins[0], inss.insert(inss.end(), ins[1].begin(), ins[1].end());
        pileup_merge_sorted(dels), pileup_merge_sorted(inss);
        out.cand_pos.push_back(pos), out.cand_depth.push_back(s.depth);
        pileup_print(out.text, pos, s.depth, s.ref_base, s.r, x, dels, inss, s.ref_count - s.del_count - s.ins_count, ref_at, cfg.max_indel_length);
    }
}

}  // namespace c3
