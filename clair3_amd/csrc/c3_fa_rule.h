// c3_fa_rule.h -- full alignment from reads, the rule: what calculate_clair3_full_alignment (src/clair3_full_alignment_dwell.c:437-1054) makes
// of the records htslib hands it, restated over aligned reads as arrays (c3_read_set, c3_read_extras, include/c3hip.h).  Plain host C++: no
// HIP, no library; it compiles into a stand-alone program as it is (tests/host/fa_reads_host_check.cpp).  The including file provides fail()
// and includes c3_pileup_rule.h's neighbours as needed.  The functions marked C3_FA_HD are the one statement of the per-read and per-cell
// arithmetic: the host form below and the kernels of c3_fa_reads.h both call them.
//
// OUTPUT per candidate: its occupied rows (33 x 8 int8 each) and their number.  The dense window is that run placed from row
// (matrix_depth - count) / 2 on (:139-150, prefix_padding_depth = padding_depth >> 1): what c3_predict_submit_rows with row_first == NULL expands.
// READ FILTER (:537-545, :547-559, :617): dropped are a read with flag & 2316, one with mapq < min_mq, one whose name_key was seen on an
//   earlier read that passed those two (first occurrence wins; no name_key: no filter), and one that covers no flanking position of any
//   candidate (it can be in no window; it is not counted as dropped).  Reads must be in coordinate order: the reference's `break` at :808 and
//   its index tiebreak rely on it; unsorted reads are refused.
// PER READ AND FLANKING POSITION p (:654-765), p inside the read's span [pos, end):
//   M, =, X over p: the base (nt16 code) and bq = normalize_bq(qual) = 100 * q / 40 below 40, else 100 (the reference divides in double and
//     truncates; for integers below 40 that is the integer quotient).
//   D over p: a deleted position; its cell stays zero (:837-842), it counts in the centre depth (:716).
//   An I op attaches to ref_pos - 1, the last reference position in front of it (:725), a D op's LENGTH likewise (:692).  P, S, H ops in
//     between change nothing.  An I in front of the read's first reference position attaches to nothing (:726 flanking_index >= flanking_start).
//   D DIRECTLY FOLLOWED BY I: the I attaches to the last deleted position.  That cell is a deleted one, so the insertion is never shown
//     (channels 1 and 6), but it IS counted in the centre's insertion counter and taken off ref_count (:751, :969).  Kept.
//   I FOLLOWED BY D: both attach to one position; the cell shows the insertion (:855 is tested first), both are counted.  Kept.
//   TWO CONSECUTIVE I OPS: the cell keeps the LAST string (:729 overwrites), the counter counts each op under its own string (:751).  Kept.
// ROWS OF A CANDIDATE c (:801-816, hap_cmp): the kept reads with pos < c + 17 and end > c - 16, ordered by (haplotype value, read index).
// CELL CHANNELS (:847-904) of a shown cell (a base of the read): 0 ref_v = num2countbase_fa of the upper-cased reference byte; 1 alt_v: -50
//   with an insertion attached, else -100 with a deletion attached, else num2countbase_fa of the read base if it differs from the reference
//   base, else 0; 2 strand (50 reverse, 100 forward); 3 normalize_mq; 4 bq; 7 HAP_TYPE = {60, 30, 90}.
// CHANNEL 6 (:855-870): an insertion at a shown cell of column p < 32 writes its bases to columns p .. p + min(len, 33 - p) - 1, columns in
//   ascending p: column c holds the base of the insertion with the LARGEST p <= c whose span reaches c.  These writes also land in cells
//   whose other channels are zero (deleted cells, cells behind the read's end).
// CHANNEL 5 (:916-948): for a row whose centre cell is shown and carries an insertion (count of its string among ALL kept reads at the
//   centre), else a deletion (count of its length), else a mismatch (acgt_count of its base): af = normalize_af(count / (float)depth),
//   float32 division and multiplication exactly as written, depth the centre depth over all kept reads; when af > 0 it goes to every cell of
//   the row whose channel 0 is non-zero.  fa_af() is the one function; no contraction can form (a division and a product, no sum).
// ALT-INFO (:950-1006): "<c + 1>-<depth>-<ref>-", X entries of the non-reference bases, R<ref> n when ref_count minus every insertion and
//   deletion counted at the centre (any length) is > 0; I and D entries of lengths <= max_indel_length.
//   DEVIATION: the reference prints I then D entries in khash order (unspecified).  Here the entries stand in the order of c3_pileup_result's
//   text: X, D by length, I by length then bytes, R (pileup_print of c3_pileup_rule.h prints both).
// DEVIATIONS, deliberate:
//  (a) MORE OVERLAPPING READS THAN matrix_depth: the reference shuffles with an unseeded process-global rand() (:121-134), so its choice
//      depends on how many deep candidates the process met before; its Python path uses yet another rule.  Here the matrix_depth reads with
//      the smallest keys fa_key(seed, centre, read index) are kept, ties by index -- the SplitMix64 counter hash and the (key, index) ranking
//      of subsample mode (c3_subsample.h subsample_mix) -- and then ordered as above.  The read index is the read's index in the read set.
//  (b) OUT-OF-SPAN CELLS: the reference reads pos_info[offset] before it checks offset (:837-845) and indexes its tables with '=' for a
//      position inside an N op.  Here a position outside the read's span is a zero cell, and a kept read with an N op over a flanking
//      position of a candidate makes the call fail with C3_FA_ERR_REFSKIP.
//  (c) NON-ACGT BASES: kept as the tables give them: acgt2num maps every letter but C, G, T to A's counter; num2countbase_fa gives N 100,
//      'D' (nt16 code 13) -100, every other letter 0.  The tables are indexed with letter - 'A'; for a byte outside 'A' .. 'A' + 31 (the
//      nt16 code 0, '=', or a reference byte that is no letter) the reference reads out of bounds: here such a byte gives 0 / A.
// HAPLOTYPES are an input of this rule; haplotag_read with its Levenshtein realignment (:262-422) is stated in c3_hap_rule.h, and
//   c3_fa_reads_phased (c3_hap_reads.h) runs it in front of this rule in one call.
// THE DWELL CHANNEL (channel 8 of the 9-channel windows, from the reads' move tables) is stated in c3_dwell_rule.h; c3_fa_reads_dwell
//   (c3_dwell.h) builds such windows with this rule for channels 0 .. 7, which it leaves as they are.
// NOT BUILT: reading BAM files.  matrix_depth may be 1 .. 128 (the reference's are 89 and 55).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>
#include "c3_pileup_rule.h"

#if defined(__HIPCC__)
#define C3_FA_HD __host__ __device__ __forceinline__
#else
#define C3_FA_HD inline
#endif

namespace c3 {

constexpr int kFaFlank = 16, kFaPositions = 33, kFaChannels = 8, kFaRowBytes = kFaPositions * kFaChannels;
constexpr int kFaMaxDepth = 128;
constexpr uint32_t kFaDropFlags = 2316;  // SAMTOOLS_VIEW_FILTER_FLAG
constexpr int64_t kFaMaxCandidates = (int64_t)1 << 24;

// what both forms read: the read set with offset tables rebased to 0, the per-op table, the per-read ends
struct FaView {
    int64_t n_reads;
    const int64_t *pos, *cigar_first, *seq_first, *qual_first, *read_end, *premax;  // premax[r] = max(read_end[0 .. r])
    const uint32_t *cigar;
    const uint16_t *flag;
    const uint8_t *mapq, *seq, *qual, *hap, *kept;
    const int64_t *op_rpos;  // per op: the reference position it starts at
    const int32_t *op_q;     // ... and the query offset
    const uint8_t *ref;      // ref[i]: the reference at ref_first + i
    int64_t ref_first;
};

C3_FA_HD int fa_table_index(int c) { return (c >= 'A' && c < 'A' + 32) ? c - 'A' : -1; }
C3_FA_HD int fa_count_base(int c) {  // num2countbase_fa[c - 'A']
    return c == 'A' ? 100 : c == 'C' ? 25 : c == 'D' ? -100 : c == 'G' ? 75 : c == 'I' ? -50 : c == 'N' ? 100 : c == 'T' ? 50 : 0;
}
C3_FA_HD int fa_acgt(int c) { return c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0; }  // acgt2num[c - 'A']
C3_FA_HD int fa_upper(int c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }
C3_FA_HD int fa_nt16_char(int code) { return "=ACMGRSVTWYHKDBN"[code & 15]; }
C3_FA_HD int fa_norm_bq(int q) { return q < 40 ? 100 * q / 40 : 100; }
C3_FA_HD int fa_norm_mq(int q) { return q < 60 ? 100 * q / 60 : 100; }
C3_FA_HD int fa_hap_v(int h) { return h == 1 ? 30 : h == 2 ? 90 : 60; }
// normalize_af(count / (float)depth): float32 quotient, float32 product with 100, truncation
C3_FA_HD int fa_af(int32_t count, int32_t depth) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float x = __fdiv_rn((float)count, (float)depth);
    return x < 1.0f ? (int)__fmul_rn(100.0f, x) : 100;
#else
    const volatile float x = (float)count / (float)depth;
    const volatile float y = 100.0f * x;
    return x < 1.0f ? (int)y : 100;
#endif
}
C3_FA_HD uint64_t fa_mix(uint64_t z) {  // subsample_mix of c3_subsample.h
    z ^= z >> 30, z *= 0xBF58476D1CE4E5B9ull, z ^= z >> 27, z *= 0x94D049BB133111EBull, z ^= z >> 31;
    return z;
}
C3_FA_HD uint64_t fa_key(uint64_t seed, int64_t centre, int64_t read) {
    return fa_mix(fa_mix(seed + 0x9E3779B97F4A7C15ull * (1 + (uint64_t)centre)) + 0x9E3779B97F4A7C15ull * (1 + (uint64_t)read));
}

// the reads that can overlap the window of centre c: [lo, hi) -- hi: the first read with pos >= c + 17; lo: the first with premax > c - 16
C3_FA_HD void fa_bounds(const FaView &v, int64_t c, int64_t *lo, int64_t *hi) {
    int64_t a = 0, b = v.n_reads;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (v.pos[m] >= c + kFaFlank + 1) b = m;
        else a = m + 1;
    }
    *hi = a;
    a = 0, b = *hi;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (v.premax[m] > c - kFaFlank) b = m;
        else a = m + 1;
    }
    *lo = a;
}
C3_FA_HD bool fa_overlaps(const FaView &v, int64_t r, int64_t c) { return v.kept[r] && v.read_end[r] > c - kFaFlank; }  // (r < hi: pos < c + 17)

// read r at reference position at
struct FaPos {
    int state;  // 0 outside the span (or inside an N op), 1 a base, 2 deleted
    int code, bq;
    int32_t q;  // the query offset of the base (state 1)
    int32_t ins_first, ins_k, ins_len, ins_q;  // the first and the LAST I op attached (-1: none), the last one's length and query offset
    int32_t del_k, del_len;                    // the D op attached (-1: none)
    int32_t next;                              // the op behind the attached run (the read's op count: none)
};
C3_FA_HD FaPos fa_pos(const FaView &v, int64_t r, int64_t at) {
    FaPos f;
    f.state = 0, f.code = 0, f.bq = 0, f.q = 0, f.ins_first = f.ins_k = f.del_k = -1, f.ins_len = f.ins_q = f.del_len = 0, f.next = 0;
    if (at < v.pos[r] || at >= v.read_end[r]) return f;
    int64_t a = v.cigar_first[r], b = v.cigar_first[r + 1];
    const int64_t c1 = b;
    while (b - a > 1) {  // the last op that starts at or in front of `at`: the op that consumes it (ops that consume no reference share
        const int64_t m = (a + b) >> 1;  // their position with the consuming op behind them)
        if (v.op_rpos[m] <= at) a = m;
        else b = m;
    }
    const uint32_t c = v.cigar[a];
    const int op = (int)(c & 15);
    const int64_t rp = v.op_rpos[a], len = c >> 4;
    if (pileup_op_base(op)) {
        const int64_t q = v.op_q[a] + (at - rp);
        f.state = 1, f.q = (int32_t)q, f.code = pileup_code(v.seq, v.seq_first[r], q), f.bq = fa_norm_bq(v.qual[v.qual_first[r] + q]);
    } else if (op == kOpD) f.state = 2;
    f.next = (int32_t)c1;
    if (at != rp + len - 1) return f;
    int64_t j = a + 1;
    for (; j < c1 && !pileup_op_ref((int)(v.cigar[j] & 15)); ++j)
        if ((int)(v.cigar[j] & 15) == kOpI) {
            if (f.ins_first < 0) f.ins_first = (int32_t)j;
            f.ins_k = (int32_t)j, f.ins_len = (int32_t)(v.cigar[j] >> 4), f.ins_q = v.op_q[j];
        }
    f.next = (int32_t)j;
    if (j < c1 && (int)(v.cigar[j] & 15) == kOpD) f.del_k = (int32_t)j, f.del_len = (int32_t)(v.cigar[j] >> 4);
    return f;
}
// two I ops hold the same string: bases are compared, nothing rests on a hash
C3_FA_HD bool fa_ins_equal(const FaView &v, int64_t ra, int64_t ka, int64_t rb, int64_t kb) {
    const int32_t len = (int32_t)(v.cigar[ka] >> 4);
    if (len != (int32_t)(v.cigar[kb] >> 4)) return false;
    const int64_t sa = v.seq_first[ra], sb = v.seq_first[rb], qa = v.op_q[ka], qb = v.op_q[kb];
    for (int32_t i = 0; i < len; ++i)
        if (pileup_code(v.seq, sa, qa + i) != pileup_code(v.seq, sb, qb + i)) return false;
    return true;
}
// the alt-info a row's centre cell carries: 1 insertion, 2 deletion, 3 mismatch, 0 none
C3_FA_HD int fa_centre_kind(const FaPos &f, int ref_char) {
    if (f.state != 1) return 0;
    if (f.ins_k >= 0) return 1;
    if (f.del_k >= 0) return 2;
    return ref_char != fa_nt16_char(f.code) ? 3 : 0;
}
// channel 6 of column c from the row's insertions at shown cells (len 0: none), ins_len / ins_q by column
C3_FA_HD int fa_ch6(const FaView &v, int64_t r, const int32_t *ins_len, const int32_t *ins_q, int c) {
    for (int p = c < kFaPositions - 2 ? c : kFaPositions - 2; p >= 0; --p)
        if (ins_len[p] > 0 && p + ins_len[p] > c) return fa_count_base(fa_nt16_char(pileup_code(v.seq, v.seq_first[r], (int64_t)ins_q[p] + (c - p))));
    return 0;
}
// the 8 bytes of a cell, channel 0 in the lowest byte
C3_FA_HD uint64_t fa_cell(const FaView &v, int64_t r, int64_t at, const FaPos &f, int af, int ch6) {
    uint64_t out = (uint64_t)(uint8_t)(int8_t)ch6 << 48;
    if (f.state != 1) return out;
    const int ref_char = fa_upper(v.ref[at - v.ref_first]);
    const int ref_v = fa_count_base(ref_char);
    const int alt_v = f.ins_k >= 0 ? -50 : f.del_k >= 0 ? -100 : ref_char != fa_nt16_char(f.code) ? fa_count_base(fa_nt16_char(f.code)) : 0;
    const int strand = (v.flag[r] & 16) ? 50 : 100;
    out |= (uint64_t)(uint8_t)(int8_t)ref_v | (uint64_t)(uint8_t)(int8_t)alt_v << 8 | (uint64_t)(uint8_t)strand << 16;
    out |= (uint64_t)(uint8_t)fa_norm_mq(v.mapq[r]) << 24 | (uint64_t)(uint8_t)f.bq << 32 | (uint64_t)(uint8_t)fa_hap_v(v.hap[r]) << 56;
    if (af > 0 && ref_v != 0) out |= (uint64_t)(uint8_t)af << 40;
    return out;
}

// ------------------------------------------------------------------------------------------ checks and tables (host, both forms)
struct FaIndel {  // an I or D op of a kept read that attaches to a position: what the text is printed from
    int64_t at;
    int32_t k, read, q, len;  // k: the op's index in the rebased cigar
    uint8_t ins;
};
struct FaTables {
    std::vector<int64_t> cfirst, sfirst, qfirst, read_end, premax, op_rpos;
    std::vector<int32_t> op_q;
    std::vector<uint8_t> kept;
    std::vector<FaIndel> indels;
    int64_t n_kept = 0, n_dropped = 0, n_ops = 0, c_base = 0, s_base = 0, q_base = 0;
};
static bool fa_in_window(const int64_t *centres, int64_t n_cand, int64_t lo, int64_t hi) {  // does [lo, hi) hold a flanking position?
    const int64_t *c = std::lower_bound(centres, centres + n_cand, lo - kFaFlank);  // the first centre whose window ends at or behind lo
    return c != centres + n_cand && *c - kFaFlank < hi;
}
// everything the rule relies on; fills the tables.  Returns 0, 1, or C3_FA_ERR_REFSKIP
static int fa_check(const c3_read_set *rs, const c3_read_extras *ex, const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first,
                    int64_t ref_len, const c3_fa_config *cfg, FaTables &t) {
    if (!cfg) return fail("fa_reads: null config");
    if (cfg->matrix_depth < 1 || cfg->matrix_depth > kFaMaxDepth) return fail("fa_reads: matrix_depth %d outside 1 .. %d", cfg->matrix_depth, kFaMaxDepth);
    if (cfg->max_indel_length < 0 || cfg->max_indel_length > (1 << 20)) return fail("fa_reads: max_indel_length %d outside 0 .. 2^20", cfg->max_indel_length);
    if (cfg->min_mq < 0 || cfg->lds_reads < 0) return fail("fa_reads: a negative min_mq or lds_reads");
    if (!rs || !ex) return fail("fa_reads: null read set or extras");
    if (n_cand < 0 || n_cand > kFaMaxCandidates) return fail("fa_reads: %lld candidates (at most %lld a call)", (long long)n_cand, (long long)kFaMaxCandidates);
    if (n_cand > 0 && !centres) return fail("fa_reads: null centres");
    for (int64_t i = 0; i < n_cand; ++i) {
        if (centres[i] < kFaFlank) return fail("fa_reads: candidate %lld at %lld lies below %d", (long long)i, (long long)centres[i], kFaFlank);
        if (i > 0 && centres[i] <= centres[i - 1]) return fail("fa_reads: candidates are not strictly ascending at %lld", (long long)i);
    }
    if (n_cand > 0 && (!ref_bytes || ref_len < 0 || ref_first < 0 || ref_first > centres[0] - kFaFlank ||
                       ref_first + ref_len <= centres[n_cand - 1] + kFaFlank + cfg->max_indel_length))
        return fail("fa_reads: the reference bytes [%lld, %lld) do not cover [%lld, %lld] (the windows and max_indel_length behind the last)",
                    (long long)ref_first, (long long)(ref_first + ref_len), (long long)(centres[0] - kFaFlank),
                    (long long)(centres[n_cand - 1] + kFaFlank + cfg->max_indel_length));
    const int64_t n = rs->n_reads;
    if (n < 0 || n > INT32_MAX) return fail("fa_reads: %lld reads", (long long)n);
    t = FaTables();
    t.cfirst.assign((size_t)n + 1, 0), t.sfirst.assign((size_t)n + 1, 0), t.qfirst.assign((size_t)n + 1, 0);
    t.read_end.assign((size_t)n, 0), t.premax.assign((size_t)n, 0), t.kept.assign((size_t)n, 0);
    if (n == 0) return 0;
    if (!rs->pos || !rs->flag || !rs->mapq || !rs->cigar_first || !rs->seq_first || !ex->qual_first || !ex->haplotype) return fail("fa_reads: a null array in the read set or the extras");
    if (rs->cigar_first[0] < 0 || rs->seq_first[0] < 0 || ex->qual_first[0] < 0) return fail("fa_reads: a negative first offset");
    for (int64_t r = 0; r < n; ++r) {
        if (rs->cigar_first[r + 1] < rs->cigar_first[r] || rs->seq_first[r + 1] < rs->seq_first[r] || ex->qual_first[r + 1] < ex->qual_first[r])
            return fail("fa_reads: an offset table is not non-decreasing at read %lld", (long long)r);
        if (rs->pos[r] < 0) return fail("fa_reads: read %lld has a negative position", (long long)r);
        if (r > 0 && rs->pos[r] < rs->pos[r - 1]) return fail("fa_reads: the reads are not in coordinate order at read %lld", (long long)r);
        if (ex->haplotype[r] > 2) return fail("fa_reads: read %lld has the haplotype %d (0, 1 or 2 expected)", (long long)r, (int)ex->haplotype[r]);
    }
    t.c_base = rs->cigar_first[0], t.s_base = rs->seq_first[0], t.q_base = ex->qual_first[0];
    t.n_ops = rs->cigar_first[n] - t.c_base;
    if (t.n_ops > INT32_MAX) return fail("fa_reads: %lld CIGAR ops in one call", (long long)t.n_ops);
    if (t.n_ops > 0 && !rs->cigar) return fail("fa_reads: null cigar");
    if (rs->seq_first[n] > t.s_base && !rs->seq) return fail("fa_reads: null seq");
    if (ex->qual_first[n] > t.q_base && !ex->qual) return fail("fa_reads: null qual");
    t.op_rpos.resize((size_t)t.n_ops), t.op_q.resize((size_t)t.n_ops);
    std::unordered_set<uint64_t> names;
    int64_t top = INT64_MIN;
    for (int64_t r = 0; r < n; ++r) {
        t.cfirst[(size_t)r + 1] = rs->cigar_first[r + 1] - t.c_base, t.sfirst[(size_t)r + 1] = rs->seq_first[r + 1] - t.s_base;
        t.qfirst[(size_t)r + 1] = ex->qual_first[r + 1] - t.q_base;
        bool kept = !(rs->flag[r] & kFaDropFlags) && (int32_t)rs->mapq[r] >= cfg->min_mq;
        if (kept && ex->name_key) kept = names.insert(ex->name_key[r]).second;
        int64_t rp = rs->pos[r], q = 0, anchor = -1;  // anchor: the last reference position consumed
        const size_t first_indel = t.indels.size();
        bool refskip = false;
        for (int64_t k = t.cfirst[(size_t)r]; k < t.cfirst[(size_t)r + 1]; ++k) {
            const uint32_t c = rs->cigar[t.c_base + k];
            const int op = (int)(c & 15);
            const int64_t len = c >> 4;
            if (op > kOpX) return fail("fa_reads: read %lld has the CIGAR op code %d", (long long)r, op);
            if (len == 0) return fail("fa_reads: read %lld has a CIGAR op of length 0", (long long)r);
            t.op_rpos[(size_t)k] = rp, t.op_q[(size_t)k] = (int32_t)q;
            if (kept && anchor >= 0 && (op == kOpI || op == kOpD)) t.indels.push_back(FaIndel{anchor, (int32_t)k, (int32_t)r, (int32_t)q, (int32_t)len, (uint8_t)(op == kOpI)});
            if (kept && op == kOpN && fa_in_window(centres, n_cand, rp, rp + len)) refskip = true;
            if (pileup_op_ref(op)) rp += len, anchor = rp - 1;
            if (pileup_op_query(op)) q += len;
            if (rp - rs->pos[r] > INT32_MAX || q > INT32_MAX) return fail("fa_reads: read %lld is longer than 2^31", (long long)r);
        }
        if (q > 2 * (rs->seq_first[r + 1] - rs->seq_first[r]) || q > ex->qual_first[r + 1] - ex->qual_first[r])
            return fail("fa_reads: the CIGAR of read %lld consumes %lld bases, its seq holds %lld and its qual %lld", (long long)r, (long long)q,
                        (long long)(2 * (rs->seq_first[r + 1] - rs->seq_first[r])), (long long)(ex->qual_first[r + 1] - ex->qual_first[r]));
        if (refskip) return fail("fa_reads: read %lld has an N op over a flanking position of a candidate", (long long)r), C3_FA_ERR_REFSKIP;
        t.read_end[(size_t)r] = rp, top = std::max(top, rp), t.premax[(size_t)r] = top;
        kept ? ++t.n_kept : ++t.n_dropped;
        // a kept read that covers no flanking position is in no window (:617); its indels attach to no centre
        if (kept && !fa_in_window(centres, n_cand, rs->pos[r], rp)) kept = false, t.indels.resize(first_indel);
        t.kept[(size_t)r] = kept;
    }
    return 0;
}
static FaView fa_view(const c3_read_set *rs, const c3_read_extras *ex, const FaTables &t, const uint8_t *ref, int64_t ref_first) {
    FaView v{};
    v.n_reads = rs->n_reads, v.pos = rs->pos, v.flag = rs->flag, v.mapq = rs->mapq, v.hap = ex->haplotype;
    v.cigar_first = t.cfirst.data(), v.seq_first = t.sfirst.data(), v.qual_first = t.qfirst.data(), v.read_end = t.read_end.data(), v.premax = t.premax.data();
    v.cigar = rs->cigar ? rs->cigar + t.c_base : nullptr, v.seq = rs->seq ? rs->seq + t.s_base : nullptr, v.qual = ex->qual ? ex->qual + t.q_base : nullptr;
    v.kept = t.kept.data(), v.op_rpos = t.op_rpos.data(), v.op_q = t.op_q.data(), v.ref = ref, v.ref_first = ref_first;
    return v;
}

// ------------------------------------------------------------------------------------------ the held result, the text, the host form
struct FaResult {
    int32_t matrix_depth = 0, channels = kFaChannels;  // channels: 8, or 9 with the dwell channel (c3_dwell_rule.h)
    std::vector<int8_t> rows;
    std::vector<int32_t> count, depth;
    std::string text;
    void clear() { *this = FaResult(); }
};
struct FaCentre {  // 24 bytes: the centre tallies of a candidate
    int32_t depth, acgt[4], pad;
};
// the lines from the centre tallies and, per attaching I / D op, the number of its equals at its centre where it is the first of them (0
// elsewhere): the device form's records, and what the host form below makes of its own tallies
static void fa_text(const c3_read_set *rs, const FaTables &t, const int64_t *centres, int64_t n_cand, const FaCentre *centre, const uint32_t *ev_count,
                    const uint8_t *ref, int64_t ref_first, int32_t max_indel_length, std::string &text) {
    std::vector<std::vector<PileupAllele>> ins((size_t)n_cand), del((size_t)n_cand);
    for (const FaIndel &e : t.indels) {
        if (!ev_count[e.k]) continue;
        const int64_t *c = std::lower_bound(centres, centres + n_cand, e.at);
        if (c == centres + n_cand || *c != e.at) continue;  // (a record stands at a centre by construction)
        PileupAllele a;
        a.len = e.len, a.count = ev_count[e.k];
        if (e.ins) a.bases = pileup_bases(rs, e.read, e.q, e.len);
        (e.ins ? ins : del)[(size_t)(c - centres)].push_back(std::move(a));
    }
    text.clear();
    for (int64_t i = 0; i < n_cand; ++i) {
        pileup_merge_sorted(ins[(size_t)i]), pileup_merge_sorted(del[(size_t)i]);
        const uint8_t *ref_at = ref + (centres[i] - ref_first);
        const int ref_char = fa_upper(*ref_at), r = fa_acgt(ref_char);
        int64_t ref_count = centre[i].acgt[r];
        for (const PileupAllele &a : ins[(size_t)i]) ref_count -= a.count;
        for (const PileupAllele &a : del[(size_t)i]) ref_count -= a.count;
        pileup_print(text, centres[i], centre[i].depth, (uint8_t)ref_char, r, centre[i].acgt, del[(size_t)i], ins[(size_t)i],
                     (int32_t)std::max<int64_t>(ref_count, 0), ref_at, max_indel_length);
    }
}

C3_FA_HD int fa_dwell_value(const FaView &v, const int32_t *cum, int64_t r, const FaPos &f);  // c3_dwell_rule.h

// the rule, candidate by candidate.  Checked input only (fa_check).  cum: the reads' dwell tables (c3_dwell_rule.h); with them a cell has a
// ninth byte
static void fa_rule_host(const c3_read_set *rs, const FaTables &t, const FaView &v, const int64_t *centres, int64_t n_cand, const c3_fa_config &cfg,
                         FaResult &out, int64_t *deep_windows, const int32_t *cum = nullptr) {
    out.clear();
    out.matrix_depth = cfg.matrix_depth, out.channels = cum ? kFaChannels + 1 : kFaChannels;
    const size_t ch = (size_t)out.channels;
    out.count.assign((size_t)n_cand, 0), out.depth.assign((size_t)n_cand, 0);
    std::vector<FaCentre> centre((size_t)n_cand);
    std::vector<uint32_t> ev_count((size_t)t.n_ops, 0);
    std::vector<int64_t> cov, sel;
    std::vector<uint64_t> key;
    std::vector<FaPos> at_centre;
    *deep_windows = 0;
    for (int64_t i = 0; i < n_cand; ++i) {
        const int64_t c = centres[i];
        int64_t lo, hi;
        fa_bounds(v, c, &lo, &hi);
        cov.clear();
        for (int64_t r = lo; r < hi; ++r)
            if (fa_overlaps(v, r, c)) cov.push_back(r);
        // the centre of every overlapping read: depth, base counts, the attached indels and how often each occurs
        FaCentre &ce = centre[(size_t)i];
        ce = FaCentre{};
        at_centre.resize(cov.size());
        for (size_t j = 0; j < cov.size(); ++j) {
            const FaPos f = at_centre[j] = fa_pos(v, cov[j], c);
            ce.depth += f.state != 0;
            if (f.state == 1) ++ce.acgt[fa_acgt(fa_nt16_char(f.code))];
        }
        auto ins_count = [&](int64_t ra, int64_t ka, bool *first) {  // over every attached I op of every overlapping read
            int32_t n = 0;
            for (size_t j = 0; j < cov.size(); ++j)
                for (int64_t k = at_centre[j].ins_first; k >= 0 && k < at_centre[j].next; ++k)
                    if ((int)(v.cigar[k] & 15) == kOpI && fa_ins_equal(v, ra, ka, cov[j], k)) {
                        ++n;
                        if (cov[j] < ra || (cov[j] == ra && k < ka)) *first = false;
                    }
            return n;
        };
        auto del_count = [&](int64_t ra, int32_t len, bool *first) {
            int32_t n = 0;
            for (size_t j = 0; j < cov.size(); ++j)
                if (at_centre[j].del_k >= 0 && at_centre[j].del_len == len) ++n, *first = *first && cov[j] >= ra;
            return n;
        };
        for (size_t j = 0; j < cov.size(); ++j) {
            const FaPos &f = at_centre[j];
            for (int64_t k = f.ins_first; k >= 0 && k < f.next; ++k)
                if ((int)(v.cigar[k] & 15) == kOpI) {
                    bool first = true;
                    const int32_t n = ins_count(cov[j], k, &first);
                    if (first) ev_count[(size_t)k] = (uint32_t)n;
                }
            if (f.del_k >= 0) {
                bool first = true;
                const int32_t n = del_count(cov[j], f.del_len, &first);
                if (first) ev_count[(size_t)f.del_k] = (uint32_t)n;
            }
        }
        // deviation (a): the matrix_depth reads of smallest (key, index)
        sel = cov;
        if ((int64_t)cov.size() > cfg.matrix_depth) {
            ++*deep_windows;
            key.resize(cov.size());
            for (size_t j = 0; j < cov.size(); ++j) key[j] = fa_key(cfg.seed, c, cov[j]);
            sel.clear();
            for (size_t j = 0; j < cov.size(); ++j) {
                int64_t rank = 0;
                for (size_t o = 0; o < cov.size(); ++o) rank += key[o] < key[j] || (key[o] == key[j] && o < j);
                if (rank < cfg.matrix_depth) sel.push_back(cov[j]);
            }
        }
        std::stable_sort(sel.begin(), sel.end(), [&](int64_t a, int64_t b) { return v.hap[a] < v.hap[b]; });  // (sel is ascending in index)
        out.count[(size_t)i] = (int32_t)sel.size(), out.depth[(size_t)i] = ce.depth;
        const int ref_char = fa_upper(v.ref[c - v.ref_first]);
        for (int64_t r : sel) {
            const FaPos fc = fa_pos(v, r, c);
            int af = 0;
            bool unused = true;
            switch (fa_centre_kind(fc, ref_char)) {
            case 1: af = fa_af(ins_count(r, fc.ins_k, &unused), ce.depth); break;
            case 2: af = fa_af(del_count(r, fc.del_len, &unused), ce.depth); break;
            case 3: af = fa_af(ce.acgt[fa_acgt(fa_nt16_char(fc.code))], ce.depth); break;
            }
            FaPos f[kFaPositions];
            int32_t ins_len[kFaPositions], ins_q[kFaPositions];
            for (int p = 0; p < kFaPositions; ++p) {
                f[p] = fa_pos(v, r, c - kFaFlank + p);
                const bool shown = f[p].state == 1 && f[p].ins_k >= 0;
                ins_len[p] = shown ? f[p].ins_len : 0, ins_q[p] = shown ? f[p].ins_q : 0;
            }
            const size_t base = out.rows.size();
            out.rows.resize(base + kFaPositions * ch);
            for (int p = 0; p < kFaPositions; ++p) {
                const uint64_t cell = fa_cell(v, r, c - kFaFlank + p, f[p], af, fa_ch6(v, r, ins_len, ins_q, p));
                for (int b = 0; b < 8; ++b) out.rows[base + (size_t)p * ch + b] = (int8_t)(cell >> (8 * b));
                if (cum) out.rows[base + (size_t)p * ch + 8] = (int8_t)fa_dwell_value(v, cum, r, f[p]);
            }
        }
    }
    fa_text(rs, t, centres, n_cand, centre.data(), ev_count.data(), v.ref, v.ref_first, cfg.max_indel_length, out.text);
}

}  // namespace c3

#include "c3_dwell_rule.h"  // (fa_dwell_value, declared above, is defined there)
