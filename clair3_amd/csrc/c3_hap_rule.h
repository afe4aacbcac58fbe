// c3_hap_rule.h -- haplotagging the reads, the rule: what haplotag_read (src/clair3_full_alignment_dwell.c:315-422) with realign_read
// (:262-313), cigar_prefix_length (:158-205), get_ref_seq / get_query_seq (:207-244), update_haplotype_cost (:246-260) and src/levenshtein.c
// makes of a read and the phased heterozygous SNPs of its contig, restated over aligned reads as arrays (c3_read_set, c3_phased_variants,
// include/c3hip.h).  The reference tags a read in front of the window loop (:604-607 moves its cursor over the variants, :629-632 calls
// haplotag_read when need_haplotagging is set and the mapq reaches min_haplotag_mq, clair3_full_alignment_dwell.h:19-20); the variants are
// the struct Variant of that header (:111-118) filled by preprocess/CreateTensorFullAlignmentFromCffi.py:80-102.  Plain host C++: no HIP, no
// library; it compiles into a stand-alone program as it is (tests/host/haplotag_host_check.cpp).  The including file provides fail().  The
// functions marked C3_HAP_HD are the one statement of the per-pair arithmetic: the host form below and the kernels of c3_hap_reads.h both
// call them.
//
// INPUT: the variants of one contig as arrays: pos (0-based, STRICTLY ascending: the reference's walk is only well defined then, anything
//   else is refused), alt_base, genotype (1 = 0|1, 2 = 1|0), phase_set.  The reference's ref_base field is never read and is no input.
// WHICH READS: a read with mapq >= min_haplotag_mq (20 in the reference) gets the rule; every other read is 0; no variants: every read 0.
//   The flag, mapq and name filters of the window rule play no part here: the windows only ever look at kept reads.
// PAIRS of a read: the variants v with pos <= v < end, and v == end when an I op stands behind the read's last reference base (:352-363 does
//   not ask whether the read goes on).  A read below the mapq has no pairs.  A variant inside an N op is a pair with allele 0 (:376-385).
// THE OP THAT OWNS A VARIANT (:332-390): M, =, X and D ops own the variants inside them.  The FIRST I op standing at ref_pos == v owns v
//   (consumed = 0) and so takes it away from the op behind it; a second I op at the same place owns nothing (positions are strictly
//   ascending).  S advances the query; H and P change nothing.
// REALIGNMENT (:262-313), overhang = 10: the left context is walked backwards from the owning op over 10 reference bases, the right one
//   forwards over 11 (the variant's own base and 10 more), by cigar_prefix_length.  Kept exactly:
//   - the outputs of a walk stay 0 when the read ends before the 10 / 11 reference bases are consumed: a variant in the first 10 reference
//     bases of a read has no left context; one in the last 10 has no right context, not even its own base, and its alt string is the left
//     context with alt_base appended (alt[left_ref_bases] lands behind the copy): such a pair votes "reference" whenever the left context
//     matches, whatever base the read carries there.
//   - an N op met by a walk sets ref_bases to the full 10 / 11 without consuming them; S, H and P ops are passed over by a walk (a soft clip
//     does NOT advance the walk's query offset); the first op of a walk counts with the part of it on that side of the variant, and is
//     skipped when that part is empty.
//   - qen == qst gives allele 0.  The query is the read's nt16 letters ("=ACMGRSVTWYHKDBN").  The reference bytes are compared AS THEY ARE,
//     no upper-casing: a soft-masked byte differs from every read base.  The strings are C strings: a NUL byte of the reference ends the
//     ref string (strncpy, strlen), and the alt string with it unless alt_base lands directly behind.
//   - the distances are Levenshtein distances (src/levenshtein.c is an exact implementation); ref < alt: allele 1, ref > alt: 2, tie: 0.
// VOTE (:246-260, :394-421): allele 0 votes nothing; else +1 for the variant's phase set when allele == genotype, else -1.  Over the phase
//   sets the read touched: none, or max == 0 and min == 0 (both start at 0): tag 0; max > |min|: tag 1; else tag 2.  Nothing rests on the
//   order of the reference's hash table.
// DEVIATION, deliberate: the reference indexes its reference string unchecked.  Here a pair whose [v - 10, v + 11) is not covered by
//   ref_bytes makes the call fail before anything is queued.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "c3_pileup_rule.h"

#if defined(__HIPCC__)
#define C3_HAP_HD __host__ __device__ __forceinline__
#else
#define C3_HAP_HD inline
#endif

namespace c3 {

constexpr int kHapOverhang = 10;                    // `overhang`, clair3_full_alignment_dwell.h:19
constexpr int kHapContext = 2 * kHapOverhang + 1;   // the longest ref / alt string; a DP row has one entry more

// what both forms read: the read set with offset tables rebased to 0, the per-op table, the variants, the pairs
struct HapView {
    int64_t n_reads, n_pairs;
    const int64_t *cigar_first, *seq_first;
    const uint32_t *cigar;
    const uint8_t *seq;
    const int64_t *op_rpos;
    const int32_t *op_q;
    const uint8_t *ref;  // ref[i]: the reference at ref_first + i
    int64_t ref_first;
    const int64_t *vpos;
    const uint8_t *valt, *vgt;
    const int32_t *vps;
    const int64_t *pair_first;  // [n_reads + 1]
    const int64_t *var_first;   // [n_reads]: the variant of a read's first pair (a read below the mapq has no pairs)
};

// cigar_prefix_length (:158-205) over the ops first, first + step, ... up to (not including) stop; the first op counts with `part` bases.
// *ref_bases / *query_bases are left alone when the ops run out before `want` reference bases are consumed
C3_HAP_HD void hap_walk(const uint32_t *cigar, int64_t first, int64_t stop, int step, int64_t part, int want, int *ref_bases, int64_t *query_bases) {
    int64_t rp = 0, qp = 0;
    for (int64_t k = first; k != stop; k += step) {
        const uint32_t c = cigar[k];
        const int op = (int)(c & 15);
        const int64_t len = k == first ? part : (int64_t)(c >> 4);
        if (len == 0) continue;
        if (pileup_op_base(op)) {
            qp += len, rp += len;
            if (rp >= want) {
                *ref_bases = want, *query_bases = qp + want - rp;
                return;
            }
        } else if (op == kOpD) {
            rp += len;
            if (rp >= want) {
                *ref_bases = want, *query_bases = qp;
                return;
            }
        } else if (op == kOpI) qp += len;
        else if (op == kOpN) {
            *ref_bases = want, *query_bases = qp;
            return;
        }
    }
}

// the allele of (read r, variant vi): 0 none, 1 the reference allele, 2 the alternative.  Both edit distances in one pass over the query:
// the DP rows run along the ref / alt string (at most kHapContext bytes) and are indexed with compile-time indices only
C3_HAP_HD int hap_pair_allele(const HapView &h, int64_t r, int64_t vi) {
    const int64_t v = h.vpos[vi], c0 = h.cigar_first[r], c1 = h.cigar_first[r + 1];
    if (c0 == c1) return 0;
    int64_t a = c0, b = c1;
    while (b - a > 1) {  // the last op that starts at or in front of v
        const int64_t m = (a + b) >> 1;
        if (h.op_rpos[m] <= v) a = m;
        else b = m;
    }
    int64_t own = a;
    if (h.op_rpos[a] == v) {  // ops that consume no reference stand in front of it at the same place: the first I op among them owns v
        int64_t f = a;
        while (f > c0 && h.op_rpos[f - 1] == v) --f;
        for (int64_t k = f; k <= a; ++k)
            if ((int)(h.cigar[k] & 15) == kOpI) {
                own = k;
                break;
            }
    }
    const uint32_t oc = h.cigar[own];
    const int op = (int)(oc & 15);
    const int64_t mid = oc >> 4;
    int64_t consumed = 0, qpos = h.op_q[own];
    if (op == kOpI) consumed = 0;
    else if (pileup_op_base(op) || op == kOpD) {
        consumed = v - h.op_rpos[own];
        if (consumed >= mid) return 0;  // (behind the read's last reference base with no I op there: no pair)
        if (op != kOpD) qpos += consumed;
    } else return 0;  // inside an N op; or S / H / P at the read's end
    int lrb = 0, rrb = 0;
    int64_t lqb = 0, rqb = 0;
    hap_walk(h.cigar, own, c0 - 1, -1, consumed, kHapOverhang, &lrb, &lqb);
    hap_walk(h.cigar, own, c1, 1, consumed < mid ? mid - consumed : 0, kHapOverhang + 1, &rrb, &rqb);
    const int64_t qst = qpos - lqb, qen = qpos + rqb;
    if (qen == qst) return 0;
    const int len = lrb + rrb;
    const uint8_t *ref = h.ref + (v - lrb - h.ref_first);
    uint8_t rb[kHapContext + 1], ab[kHapContext + 1];
    const uint8_t alt_base = h.valt[vi];
#pragma unroll
    for (int j = 0; j <= kHapContext; ++j) rb[j] = j < len ? ref[j] : 0;
    int nr = len;  // strlen of the ref string
#pragma unroll
    for (int j = kHapContext; j >= 0; --j)
        if (j < len && rb[j] == 0) nr = j;
#pragma unroll
    for (int j = 0; j <= kHapContext; ++j) ab[j] = j == lrb ? alt_base : j < nr ? rb[j] : (uint8_t)0;
    int na = kHapContext + 1;  // strlen of the alt string (at most kHapContext: lrb <= 10)
#pragma unroll
    for (int j = kHapContext; j >= 0; --j)
        if (ab[j] == 0) na = j;
    int32_t dr[kHapContext + 1], da[kHapContext + 1];
#pragma unroll
    for (int j = 0; j <= kHapContext; ++j) dr[j] = da[j] = j;
    const int64_t s0 = h.seq_first[r];
    for (int64_t q = qst; q < qen; ++q) {
        const int ch = "=ACMGRSVTWYHKDBN"[pileup_code(h.seq, s0, q)];
        int32_t diag_r = dr[0], diag_a = da[0];
        dr[0] = da[0] = (int32_t)(q - qst) + 1;
#pragma unroll
        for (int j = 1; j <= kHapContext; ++j) {
            const int32_t up_r = dr[j], up_a = da[j];
            const int32_t sub_r = diag_r + (rb[j - 1] != ch), sub_a = diag_a + (ab[j - 1] != ch);
            const int32_t side_r = (up_r < dr[j - 1] ? up_r : dr[j - 1]) + 1, side_a = (up_a < da[j - 1] ? up_a : da[j - 1]) + 1;
            dr[j] = sub_r < side_r ? sub_r : side_r, da[j] = sub_a < side_a ? sub_a : side_a;
            diag_r = up_r, diag_a = up_a;
        }
    }
    int32_t dist_r = 0, dist_a = 0;
#pragma unroll
    for (int j = 0; j <= kHapContext; ++j) {
        if (j == nr) dist_r = dr[j];
        if (j == na) dist_a = da[j];
    }
    return dist_r < dist_a ? 1 : dist_r > dist_a ? 2 : 0;
}

C3_HAP_HD int hap_vote(const HapView &h, int64_t vi, int allele) { return allele == 0 ? 0 : allele == (int)h.vgt[vi] ? 1 : -1; }
C3_HAP_HD int hap_tag(bool any, int32_t max_v, int32_t min_v) {  // (:410-421)
    if (!any || (max_v == 0 && min_v == 0)) return 0;
    return max_v > (min_v < 0 ? -min_v : min_v) ? 1 : 2;
}

// ------------------------------------------------------------------------------------------ checks and tables (host, both forms)
struct HapTables {
    std::vector<int64_t> cfirst, sfirst, read_end, op_rpos, pair_first, var_first;
    std::vector<int32_t> op_q;
    int64_t n_ops = 0, n_pairs = 0, c_base = 0, s_base = 0, n_low = 0;
};
struct HapResult {
    std::vector<uint8_t> hap;
    std::vector<int8_t> alleles;
    std::vector<int64_t> pair_first;
    void clear() { *this = HapResult(); }
};

// everything the rule relies on; fills the tables.  Returns 0 or 1
static int hap_check(const c3_read_set *rs, const c3_phased_variants *vs, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                     const c3_haplotag_config *cfg, HapTables &t) {
    if (!cfg) return fail("haplotag: null config");
    if (cfg->min_haplotag_mq < 0) return fail("haplotag: a negative min_haplotag_mq");
    if (!rs || !vs) return fail("haplotag: null read set or variants");
    const int64_t n = rs->n_reads, nv = vs->n;
    if (n < 0 || n > INT32_MAX) return fail("haplotag: %lld reads", (long long)n);
    if (nv < 0 || nv > INT32_MAX) return fail("haplotag: %lld variants", (long long)nv);
    if (nv > 0 && (!vs->pos || !vs->alt_base || !vs->genotype || !vs->phase_set)) return fail("haplotag: a null array in the variants");
    for (int64_t i = 0; i < nv; ++i) {
        if (vs->pos[i] < 0) return fail("haplotag: variant %lld has a negative position", (long long)i);
        if (i > 0 && vs->pos[i] <= vs->pos[i - 1]) return fail("haplotag: the variants are not strictly ascending at %lld", (long long)i);
        if (vs->genotype[i] != 1 && vs->genotype[i] != 2) return fail("haplotag: variant %lld has the genotype %d (1 = 0|1 or 2 = 1|0 expected)", (long long)i, (int)vs->genotype[i]);
    }
    t = HapTables();
    t.cfirst.assign((size_t)n + 1, 0), t.sfirst.assign((size_t)n + 1, 0), t.pair_first.assign((size_t)n + 1, 0);
    t.read_end.assign((size_t)n, 0), t.var_first.assign((size_t)n, 0);
    if (n == 0) return 0;
    if (!rs->pos || !rs->mapq || !rs->cigar_first || !rs->seq_first) return fail("haplotag: a null array in the read set");
    if (rs->cigar_first[0] < 0 || rs->seq_first[0] < 0) return fail("haplotag: a negative first offset");
    for (int64_t r = 0; r < n; ++r) {
        if (rs->cigar_first[r + 1] < rs->cigar_first[r] || rs->seq_first[r + 1] < rs->seq_first[r])
            return fail("haplotag: an offset table is not non-decreasing at read %lld", (long long)r);
        if (rs->pos[r] < 0) return fail("haplotag: read %lld has a negative position", (long long)r);
    }
    t.c_base = rs->cigar_first[0], t.s_base = rs->seq_first[0];
    t.n_ops = rs->cigar_first[n] - t.c_base;
    if (t.n_ops > INT32_MAX) return fail("haplotag: %lld CIGAR ops in one call", (long long)t.n_ops);
    if (t.n_ops > 0 && !rs->cigar) return fail("haplotag: null cigar");
    if (rs->seq_first[n] > t.s_base && !rs->seq) return fail("haplotag: null seq");
    t.op_rpos.resize((size_t)t.n_ops), t.op_q.resize((size_t)t.n_ops);
    for (int64_t r = 0; r < n; ++r) {
        t.cfirst[(size_t)r + 1] = rs->cigar_first[r + 1] - t.c_base, t.sfirst[(size_t)r + 1] = rs->seq_first[r + 1] - t.s_base;
        int64_t rp = rs->pos[r], q = 0;
        bool tail_ins = false;  // an I op behind the last reference base
        for (int64_t k = t.cfirst[(size_t)r]; k < t.cfirst[(size_t)r + 1]; ++k) {
            const uint32_t c = rs->cigar[t.c_base + k];
            const int op = (int)(c & 15);
            const int64_t len = c >> 4;
            if (op > kOpX) return fail("haplotag: read %lld has the CIGAR op code %d", (long long)r, op);
            if (len == 0) return fail("haplotag: read %lld has a CIGAR op of length 0", (long long)r);
            t.op_rpos[(size_t)k] = rp, t.op_q[(size_t)k] = (int32_t)q;
            if (pileup_op_ref(op)) rp += len, tail_ins = false;
            else if (op == kOpI) tail_ins = true;
            if (pileup_op_query(op)) q += len;
            if (rp - rs->pos[r] > INT32_MAX || q > INT32_MAX) return fail("haplotag: read %lld is longer than 2^31", (long long)r);
        }
        if (q > 2 * (rs->seq_first[r + 1] - rs->seq_first[r]))
            return fail("haplotag: the CIGAR of read %lld consumes %lld bases, its seq holds %lld", (long long)r, (long long)q,
                        (long long)(2 * (rs->seq_first[r + 1] - rs->seq_first[r])));
        t.read_end[(size_t)r] = rp;
        int64_t lo = 0, hi = 0;
        if ((int32_t)rs->mapq[r] < cfg->min_haplotag_mq) ++t.n_low;
        else if (nv > 0) {
            lo = std::lower_bound(vs->pos, vs->pos + nv, rs->pos[r]) - vs->pos;
            hi = std::lower_bound(vs->pos, vs->pos + nv, rp + (tail_ins ? 1 : 0)) - vs->pos;
        }
        t.var_first[(size_t)r] = lo, t.pair_first[(size_t)r + 1] = t.pair_first[(size_t)r] + (hi - lo);
        if (hi > lo) {  // the deviation: every context a pair may read is covered
            const int64_t first = vs->pos[lo] - kHapOverhang, last = vs->pos[hi - 1] + kHapOverhang + 1;
            if (!ref_bytes || ref_len < 0 || first < ref_first || last > ref_first + ref_len)
                return fail("haplotag: the reference bytes [%lld, %lld) do not cover [%lld, %lld), the contexts of the variants under read %lld",
                            (long long)ref_first, (long long)(ref_first + ref_len), (long long)first, (long long)last, (long long)r);
        }
    }
    t.n_pairs = t.pair_first[(size_t)n];
    return 0;
}
static HapView hap_view(const c3_read_set *rs, const c3_phased_variants *vs, const HapTables &t, const uint8_t *ref, int64_t ref_first) {
    HapView h{};
    h.n_reads = rs->n_reads, h.n_pairs = t.n_pairs, h.cigar_first = t.cfirst.data(), h.seq_first = t.sfirst.data();
    h.cigar = rs->cigar ? rs->cigar + t.c_base : nullptr, h.seq = rs->seq ? rs->seq + t.s_base : nullptr;
    h.op_rpos = t.op_rpos.data(), h.op_q = t.op_q.data(), h.ref = ref, h.ref_first = ref_first;
    h.vpos = vs->pos, h.valt = vs->alt_base, h.vgt = vs->genotype, h.vps = vs->phase_set;
    h.pair_first = t.pair_first.data(), h.var_first = t.var_first.data();
    return h;
}

// the rule, read by read.  Checked input only (hap_check)
static void hap_rule_host(const HapView &h, HapResult &out) {
    out.clear();
    out.hap.assign((size_t)h.n_reads, 0), out.alleles.assign((size_t)h.n_pairs, 0);
    out.pair_first.assign(h.pair_first, h.pair_first + h.n_reads + 1);
    std::vector<std::pair<int32_t, int32_t>> cost;  // (phase set, sum) of the sets the read touched
    for (int64_t r = 0; r < h.n_reads; ++r) {
        cost.clear();
        for (int64_t p = h.pair_first[r]; p < h.pair_first[r + 1]; ++p) {
            const int64_t vi = h.var_first[r] + (p - h.pair_first[r]);
            const int allele = hap_pair_allele(h, r, vi);
            out.alleles[(size_t)p] = (int8_t)allele;
            if (allele == 0) continue;
            size_t k = 0;
            while (k < cost.size() && cost[k].first != h.vps[vi]) ++k;
            if (k == cost.size()) cost.emplace_back(h.vps[vi], 0);
            cost[k].second += hap_vote(h, vi, allele);
        }
        int32_t max_v = 0, min_v = 0;
        for (const auto &c : cost) max_v = std::max(max_v, c.second), min_v = std::min(min_v, c.second);
        out.hap[(size_t)r] = (uint8_t)hap_tag(!cost.empty(), max_v, min_v);
    }
}

}  // namespace c3
