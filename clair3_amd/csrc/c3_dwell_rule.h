// c3_dwell_rule.h -- the dwell channel of the full-alignment windows, the rule: what src/clair3_full_alignment_dwell.c makes of a read's
// nanopore move table (the `mv:B:c` tag) when enable_dwell_time is set, restated over the reads as arrays (c3_read_set, c3_read_extras and
// c3_read_moves, include/c3hip.h).  Plain host C++ like c3_fa_rule.h, which it completes: the functions marked C3_FA_HD are the one statement
// of the per-cell arithmetic, called by the host form (fa_rule_host of c3_fa_rule.h) and by the kernels of c3_dwell.h.
//
// SIGNAL LENGTHS OF A READ (compute_signal_lengths_from_mv_tag, :20-74).  mv[0 .. L) is the read's move table as the tag holds it; element 0
//   is the stride and is skipped (:43 starts at 1).  l is the read's query length; c3_read_set packs two bases a byte and does not state it,
//   so l is the number of quality bytes the read owns, qual_first[r + 1] - qual_first[r]: what bam_get_qual holds (:33 core.l_qseq).
//   NO TABLE (:26-35 return NULL; channel 8 of every cell of the read is then 0, :669, :734, :743): L <= 1 or l == 0.  A read without the
//     tag has L == 0.
//   OTHERWISE (:41-61) let n_0 < n_1 < .. < n_(K-1) be the indices in [1, L) with mv != 0.  ANY non-zero value counts, negative ones
//     included (:46).  sig[k] = n_(k+1) - n_k for k < K - 1 (:51 and the zeros behind it, :59); sig[K-1] = L - n_(K-1); sig[k] = 0 for
//     K <= k < l (:37 calloc).  Zeros in front of n_0 belong to nobody (:55-56).  Bases k >= l are dropped (:49-50, the `break`).
//   REVERSE (:63-71): a read with flag & 16 has sig[0 .. l) reversed, so that the index is the query position as the BAM stores the bases.
// THE TABLE both forms keep per read is the prefix array cum[0 .. l] of int32 in query order, after the reversal:
//   cum[q] = sig[0] + .. + sig[q-1].  Read r owns cum[qual_first[r] + r .. qual_first[r + 1] + r + 1) (offsets rebased to the first read); a
//   read without a table has zeros there.  A sum over query bases is a difference of two entries: no cell loops over an insertion's bases.
// CHANNEL 8 OF A CELL (:669-672, :730-744, :905-911):
//   a cell that is not a shown base is 0: positions outside the span, deleted positions (:908), the cells behind the read's end that
//     channel 6 writes into.
//   a shown cell at query offset q has s = sig[q] (:671).
//   every I op attached to the position adds sig[q_k .. q_k + len_k), clipped at l (:731-744, `+=`).  TWO CONSECUTIVE I OPS both add, where
//     channel 6 keeps only the last string.  I FOLLOWED BY D: the I adds.
//   D DIRECTLY FOLLOWED BY I: the I attaches to a deleted cell, whose value is 0 (:908).
//   an I in front of the read's first reference position attaches to nothing (:726): the attach rule of c3_fa_rule.h.
//   QUIRK, kept and named: the byte is (int8_t) of the int32 sum as the reference writes it (:910), no clamp.  A sum of 200 is stored as
//     -56, a sum of 256 as 0.  The network was trained on these bytes.
// Channels 0 .. 7, row selection, row order, counts, centre depths and the alt-info text are those of c3_fa_rule.h, with every deviation
//   listed there.
// LIMITS: no BAM is read; the caller converts any `B` subtype to int8 (only zero or non-zero matters); L < 2^31 per read.
#pragma once
#include "c3_fa_rule.h"

namespace c3 {

constexpr int kDwChannels = kFaChannels + 1, kDwRowBytes = kFaPositions * kDwChannels;  // 297

// the sequential statement, in the shape of the reference's loop: cum_out[0 .. l] of one read; returns whether a table exists
inline bool fa_dwell_cum_host(const int8_t *mv, int64_t L, int64_t l, bool reverse, int32_t *cum_out) {
    for (int64_t q = 0; q <= l; ++q) cum_out[q] = 0;
    if (L <= 1 || l == 0) return false;
    int32_t *signals = cum_out + 1;  // sig[k] stands at cum_out[k + 1] until the sums are taken
    int64_t base_index = -1;
    for (int64_t idx = 1; idx < L; ++idx) {
        if (mv[idx] != 0) {
            base_index++;
            if (base_index >= l) break;
            signals[base_index] += 1;
        } else {
            if (base_index < 0) continue;
            signals[base_index] += 1;
        }
    }
    if (reverse)
        for (int64_t i = 0, j = l - 1; i < j; ++i, --j) std::swap(signals[i], signals[j]);
    for (int64_t q = 1; q <= l; ++q) cum_out[q] += cum_out[q - 1];
    return true;
}

// channel 8 of the cell of read r that f describes, as the int32 sum; the byte is its (int8_t)
C3_FA_HD int fa_dwell_value(const FaView &v, const int32_t *cum, int64_t r, const FaPos &f) {
    if (f.state != 1) return 0;
    const int64_t q0 = v.qual_first[r], l = v.qual_first[r + 1] - q0;
    const int32_t *c = cum + q0 + r;
    int32_t s = c[f.q + 1] - c[f.q];  // (f.q < l: fa_check holds the CIGAR to the quality bytes)
    for (int64_t k = f.ins_first; k >= 0 && k < f.next; ++k)  // every attached I op, not only the last
        if ((int)(v.cigar[k] & 15) == kOpI) {
            const int64_t a = v.op_q[k], b = a + (int64_t)(v.cigar[k] >> 4);
            s += c[b < l ? b : l] - c[a < l ? a : l];
        }
    return (int)(int8_t)s;
}

// the 9 bytes of a cell: fa_cell's eight and the dwell byte
struct FaCell9 {
    uint64_t lo;
    uint8_t dwell;
};
C3_FA_HD FaCell9 fa_cell9(const FaView &v, const int32_t *cum, int64_t r, int64_t at, const FaPos &f, int af, int ch6) {
    FaCell9 c;
    c.lo = fa_cell(v, r, at, f, af, ch6), c.dwell = (uint8_t)(int8_t)fa_dwell_value(v, cum, r, f);
    return c;
}

// ------------------------------------------------------------------------------------------ checks and the table (host, both forms)
struct DwTables {
    std::vector<int64_t> mfirst;  // [n + 1] rebased to 0
    int64_t m_base = 0, n_moves = 0, n_cum = 0, n_tables = 0;
};
// everything the rule relies on in a c3_read_moves; t: the checked tables of the same reads
static int fa_dwell_check(const c3_read_moves *mv, const FaTables &t, int64_t n, DwTables &d, const char *what) {
    if (!mv) return fail("%s: null moves", what);
    d = DwTables();
    d.mfirst.assign((size_t)n + 1, 0);
    d.n_cum = t.qfirst[(size_t)n] + n;
    if (n == 0) return 0;
    if (!mv->mv_first) return fail("%s: null mv_first", what);
    if (mv->mv_first[0] < 0) return fail("%s: mv_first starts at a negative offset", what);
    d.m_base = mv->mv_first[0];
    for (int64_t r = 0; r < n; ++r) {
        const int64_t L = mv->mv_first[r + 1] - mv->mv_first[r];
        if (L < 0) return fail("%s: mv_first is not non-decreasing at read %lld", what, (long long)r);
        if (L > INT32_MAX) return fail("%s: the move table of read %lld has %lld entries", what, (long long)r, (long long)L);
        d.mfirst[(size_t)r + 1] = mv->mv_first[r + 1] - d.m_base;
        d.n_tables += L > 1 && t.qfirst[(size_t)r + 1] > t.qfirst[(size_t)r];
    }
    d.n_moves = d.mfirst[(size_t)n];
    if (d.n_moves > 0 && !mv->mv) return fail("%s: null mv", what);
    if (d.n_cum > INT32_MAX) return fail("%s: %lld quality bytes in one call", what, (long long)d.n_cum);
    return 0;
}
// the table of every read, sequentially
static void fa_dwell_tables_host(const c3_read_set *rs, const c3_read_moves *mv, const FaTables &t, const DwTables &d, std::vector<int32_t> &cum) {
    const int64_t n = rs->n_reads;
    cum.assign((size_t)d.n_cum, 0);
    for (int64_t r = 0; r < n; ++r)
        fa_dwell_cum_host(mv->mv ? mv->mv + d.m_base + d.mfirst[(size_t)r] : nullptr, d.mfirst[(size_t)r + 1] - d.mfirst[(size_t)r],
                          t.qfirst[(size_t)r + 1] - t.qfirst[(size_t)r], (rs->flag[r] & 16) != 0, cum.data() + t.qfirst[(size_t)r] + r);
}

}  // namespace c3
