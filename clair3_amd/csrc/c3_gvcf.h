// c3_gvcf.h -- the non-variant half of the reference's --gvcf: the <NON_REF> block records made from the per-site (n_ref, n_total) of the
// pileup step (preprocess/CreateTensorPileupFromCffi.py:399-441 -> preprocess/utils.py variantInfoCalculator.make_gvcf_online :398-488,
// reference_likelihood / _cal_reference_likelihood :490-568, write_to_gvcf_batch :577-606, write_to_gvcf :608-622,
// write_empty_pileup :392-397).  Host C (the sequential rule, the site record, the text) and the device path.
//
// THE SITE RECORD depends on (n_ref, n_total, reference byte) alone: gq 0 .. 50, binned_gq, gt (0/0 iff validPL, else ./.) and three integer
// PLs, all of them int() of doubles the reference rounds with round(., 6) (normalize_log10_prob, log10p_to_phred), with LOG_10 = 2.3025 and
// LOG_2 = 0.3010 as it writes them.  round(x, 6) is a correctly rounded conversion to six decimals and back: "%.6f" and strtod, both
// exact in glibc.  A byte outside upper-case ACGT prints as N with gq = binned_gq = 1 and PL 0,0,0; its gt stays what the counts say.  The
// integers come out of pow / log of the host's libm, which the device's need not equal to the last bit, so they are never computed on the
// device: the context keeps a triangular table T[n_total][n_ref] of records (it grows with the deepest site seen, up to kGvcfTableDepth
// rows, and never shrinks) that gvcf_site computes on the host; the kernels look records up.  A call with sites deeper than the table (a few
// in a genome, or a test) copies its counts back once, and the host sends the records of the distinct deep pairs as a sorted side table.
//
// THE BLOCK RULE.  make_gvcf_online starts a block where binned_gq, gt or the is-exactly-'N' status of the RAW byte differs from the
// block's first item (hard breaks), or where its DP rule fires.  "Differs from the first item" is "differs from the previous site":
// binned_gq and gt are reset by every kind of break, so inside a block all items equal the first; cur_ref alone is NOT reset by a DP break
// and may be stale, but it goes stale only inside a stretch without an N-status break, where every site has the status cur_ref has
// (the branch tests (_cur_ref != cur_ref) and (one of them is 'N'): two bytes of equal status never break, two of different status
// always do), so the stale value answers as the previous site's would.  gvcf_blocks_rule below keeps the reference's literal form, stale
// cur_ref included; the kernels and the numpy mirror use the previous site.
// The DP rule (:462-488), with f(x) = ceil(x + x * 0.3) in double: site i stays in the block that began at s iff
// max(dp[s..i]) <= f(min(dp[s..i])) -- a new minimum m breaks iff cur_max > f(m), a new maximum M stays iff M <= f(cur_min), anything
// between changes neither extreme; both are that one test on the new extremes.  The test is monotone in i, so the block from s ends at
// e(s) = the first i > s with a hard break at i or a failing test, e(s) is non-decreasing in s, and a region's blocks are the chain
// 0 -> e(0) -> e(e(0)) -> ...  A block prints MIN_DP = min dp, GQ = min of the items' gq (after the N rule), and gt, PL, ref of its first item
// (an N first item: ./., GQ 1, PL 0,0,0).  A block whose first item is ./. and not N, and every block under bp_resolution whose first
// item is not N, is written item by item, each with its own binned_gq (:579-582).
//
// COLUMN <-> POSITION (CreateTensorPileupFromCffi.py:413-423 against src/clair3_pileup.c:453): calculate_clair3_pileup files the counts of
// the 0-based position p (= plp_data.major of its column) at pos_ref_count[p - (extend_start - 1)]; the loop reads, for the 1-based site
// P it prints, index P - extend_start + offset with offset = 0 if ctg_start == 1 else 1.  So site P takes the column whose major is
// P - 1 + offset: P itself (the usual case: the counts one base to the right of the printed position, as the reference has it), or P - 1
// for a chunk that starts at 1.  The caller passes that major for its first site (first_major); site j reads major first_major + j, and
// a site without a column has 0 / 0.
//
// The launches of a call, on the context's stream (no atomics, fixed-order scans: the records do not depend on scheduling; no lane's work
// grows with the length of a block or of a run between hard breaks):
//   gvcf_counts_kernel / gvcf_region_kernel   (n_ref, n_total) of every site from the caller's arrays, or from the region matrix as
//                        calculate_clair3_pileup leaves it (:355-371, :452-455), scattered by major
//   gvcf_max_kernel      max n_total per tile (a refused count poisons it) -> host: table rows up to the maximum
//   gvcf_site_kernel     table lookup -> site record, and the leaf of the tree: dp, gq, hard break against the previous site
//   gvcf_tree_kernel     min dp / max dp / min gq / any-hard-break over aligned 2^k ranges, ten levels per launch
//   gvcf_search_kernel   e(s) for every s: up the tree while the range can be absorbed, then down: O(log n) nodes per site
//   gvcf_last_kernel     pointer doubling in LDS: the last chain element inside s's tile of kGvcfTile sites
//   gvcf_group_kernel    the same for groups of 2, 4, .. kGvcfGroupTiles tiles, one round per launch, in place
//   gvcf_entry_kernel    the chain over groups (one thread), then over the tiles of every group (one thread per group): each tile's
//                        first chain element and the block start that covers the sites in front of it
//   gvcf_mark_kernel     pointer doubling in LDS from the tile's entry: block starts; which sites are written item by item
//   gvcf_count_kernel / gvcf_scan_kernel / gvcf_emit_kernel   order-preserving compaction to c3_gvcf_block records
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

namespace c3 {

constexpr int kGvcfTile = 1024;            // sites per workgroup of the tile kernels; one tree launch builds log2 of it levels
constexpr int kGvcfTileLog = 10;
constexpr int kGvcfGroupLog = 8;           // a group = 2^8 tiles: what the one-thread-per-group walk of gvcf_entry_kernel steps through
constexpr int64_t kGvcfGroupSites = (int64_t)kGvcfTile << kGvcfGroupLog;  // the span of the top level: 262144 sites
constexpr int kGvcfTableDepth = 1024;      // rows of the device table at most (525 825 records, 8.4 MB); deeper sites: the host's records
constexpr int kGvcfMaxDepth = 65535;
constexpr int kGvcfMaxGq = 50;
constexpr int kGvcfMaxLevels = 34;

// a site record: the reference's item without chr / pos.  meta = gq | binned_gq << 8 | flags << 16 | printed ref byte << 24
struct GvcfRec {
    int32_t pl[3];
    uint32_t meta;
};
enum : uint32_t { kGvcfValid = 1u << 16, kGvcfNotAcgt = 2u << 16, kGvcfIsN = 4u << 16 };
__host__ __device__ __forceinline__ uint32_t gvcf_gq(uint32_t meta) { return meta & 255u; }
__host__ __device__ __forceinline__ uint32_t gvcf_binned(uint32_t meta) { return (meta >> 8) & 255u; }
// what a hard break compares: binned_gq, gt, the is-exactly-'N' status of the raw byte
__host__ __device__ __forceinline__ uint32_t gvcf_key(uint32_t meta) { return meta & (0xff00u | kGvcfValid | kGvcfIsN); }
// the rule of reference_likelihood :510-516 on a table record: the byte, and what a byte outside ACGT does to gq / binned_gq / PL
__host__ __device__ __forceinline__ GvcfRec gvcf_apply_ref(GvcfRec r, uint8_t ref) {
    const bool acgt = ref == 'A' || ref == 'C' || ref == 'G' || ref == 'T';
    if (!acgt) {
        r.pl[0] = r.pl[1] = r.pl[2] = 0;
        r.meta = (r.meta & kGvcfValid) | 1u | (1u << 8) | kGvcfNotAcgt | (ref == 'N' ? kGvcfIsN : 0u) | ((uint32_t)'N' << 24);
    } else r.meta = (r.meta & (0xffffu | kGvcfValid)) | ((uint32_t)ref << 24);
    return r;
}
// f(x) = ceil(x + x * 0.3) in double, one rounding per operation (never a fused multiply-add)
__host__ __device__ __forceinline__ uint32_t gvcf_f(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)ceil(__dadd_rn((double)x, __dmul_rn((double)x, 0.3)));
#else
    volatile double prod = (double)x * 0.3;
    return (uint32_t)ceil((double)x + prod);
#endif
}

// ------------------------------------------------------------------------------------------ the site record (host)
static double gvcf_round6(double x) {  // Python's round(x, 6)
    if (!std::isfinite(x)) return x;
    char b[400];
    snprintf(b, sizeof(b), "%.6f", x);
    return strtod(b, nullptr);
}

struct GvcfMath {
    double logp = 0, log1p_ = 0;
    int bin = 5;
    void set(double base_err, int gq_bin_size) {
        logp = log(base_err) / 2.3025, log1p_ = log1p(-base_err) / 2.3025;
        bin = gq_bin_size;
    }
    // mathcalculator.normalize_log10_prob with its Python log10sumexp (speedUp = False)
    static void normalize(const double in[3], double out[3]) {
        const double m = std::max(in[0], std::max(in[1], in[2]));
        double s = pow(10.0, in[0] - m);
        s += pow(10.0, in[1] - m);
        s += pow(10.0, in[2] - m);
        const double lse = gvcf_round6(m + log10(s));
        for (int i = 0; i < 3; ++i) out[i] = std::min(in[i] - lse, 0.0);
    }
    GvcfRec site(int64_t n_ref, int64_t n_total) const {
        double l[3];
        if (n_total == 0) {
            const double c[3] = {-1.0, -1.0, -1.0};
            normalize(c, l);
        } else {
            const double nr = (double)n_ref, na = (double)(n_total - n_ref);
            volatile double a = nr * log1p_, b = na * logp, c = nr * logp, d = na * log1p_;  // (each product rounded before its sum)
            const double in[3] = {a + b, (double)(-n_total) * 0.3010, c + d};
            normalize(in, l);
        }
        const double ptrue = pow(10.0, l[0]);
        const double gqd = ptrue == 1.0 ? 50.0 : gvcf_round6(-10.0 * (log(1.0 - ptrue) / 2.3025));
        const int gq = (int)std::min<double>(trunc(gqd), (double)kGvcfMaxGq);
        const int binned = gq >= 1 ? (gq - 1) / bin * bin + 1 : 0;
        const bool valid = l[0] == std::max(l[0], std::max(l[1], l[2]));
        const double t[3] = {-10.0 * l[0], -10.0 * l[1], -10.0 * l[2]};
        const double mn = std::min(t[0], std::min(t[1], t[2]));
        GvcfRec r;
        for (int i = 0; i < 3; ++i) r.pl[i] = (int32_t)(t[i] - mn);
        r.meta = (uint32_t)gq | (uint32_t)binned << 8 | (valid ? kGvcfValid : 0u);
        return r;
    }
};

// the records by (n_total, n_ref): dense rows 0 .. depth (what the device holds a copy of) and a map for deeper sites
struct GvcfTable {
    GvcfMath math;
    std::vector<GvcfRec> rows;  // T[nt * (nt + 1) / 2 + nr]
    int depth = -1;             // rows 0 .. depth are complete
    std::unordered_map<uint64_t, GvcfRec> deep;
    static size_t index(int64_t nt, int64_t nr) { return (size_t)(nt * (nt + 1) / 2 + nr); }
    static constexpr uint32_t kUnset = 0xffffffffu;  // (no record has this meta)
    void reserve_rows(int d) {
        if (index(d + 1, 0) > rows.size()) rows.resize(index(d + 1, 0), GvcfRec{{0, 0, 0}, kUnset});
    }
    // every record of rows 0 .. d (what the device's copy needs); the host's own lookups fill the rows one record at a time
    void ensure(int d) {
        d = std::min(d, kGvcfTableDepth);
        if (d <= depth) return;
        reserve_rows(d);
        for (int nt = depth + 1; nt <= d; ++nt)
            for (int nr = 0; nr <= nt; ++nr)
                if (rows[index(nt, nr)].meta == kUnset) rows[index(nt, nr)] = math.site(nr, nt);
        depth = d;
    }
    GvcfRec get(int64_t nr, int64_t nt) {
        if (nt <= kGvcfTableDepth) {
            reserve_rows((int)nt);
            GvcfRec &r = rows[index(nt, nr)];
            if (r.meta == kUnset) r = math.site(nr, nt);
            return r;
        }
        const uint64_t k = (uint64_t)nt << 32 | (uint64_t)nr;
        auto it = deep.find(k);
        if (it != deep.end()) return it->second;
        return deep[k] = math.site(nr, nt);
    }
};

static const char *gvcf_count_error(int64_t nr, int64_t nt) {
    if (nr < 0 || nt < 0) return "a negative count";
    if (nr > nt) return "n_ref > n_total";
    if (nt > kGvcfMaxDepth) return "a depth above 65535";
    return nullptr;
}

// ------------------------------------------------------------------------------------------ the sequential rule (host)
// one written record (write_to_gvcf_batch): a block, or one item of a block that is written item by item
static void gvcf_write_block(const std::vector<GvcfRec> &recs, const uint16_t *dp, int64_t s, int64_t e, int64_t first_pos, int min_dp,
                             int max_dp, int min_gq, bool bp, std::vector<c3_gvcf_block> &out) {
    const uint32_t fm = recs[s].meta;
    if ((bp || !(fm & kGvcfValid)) && !(fm & kGvcfNotAcgt)) {
        for (int64_t i = s; i <= e; ++i) {
            c3_gvcf_block b{};
            const GvcfRec &r = recs[i];
            b.pos = b.end = first_pos + i, b.min_dp = b.max_dp = dp[i], b.gq = (int32_t)gvcf_binned(r.meta);
            b.pl[0] = r.pl[0], b.pl[1] = r.pl[1], b.pl[2] = r.pl[2];
            b.ref = (uint8_t)(r.meta >> 24), b.gt = (r.meta & kGvcfValid) ? 1 : 0, b.per_site = 1, b.first_n = 0;
            out.push_back(b);
        }
        return;
    }
    c3_gvcf_block b{};
    b.pos = first_pos + s, b.end = first_pos + e, b.min_dp = min_dp, b.max_dp = max_dp;
    if (fm & kGvcfNotAcgt) b.gq = 1, b.gt = 0, b.ref = 'N', b.first_n = 1;
    else {
        b.gq = min_gq, b.gt = (fm & kGvcfValid) ? 1 : 0, b.ref = (uint8_t)(fm >> 24);
        b.pl[0] = recs[s].pl[0], b.pl[1] = recs[s].pl[1], b.pl[2] = recs[s].pl[2];
    }
    out.push_back(b);
}

// make_gvcf_online :398-488 as it stands, the stale cur_ref included
static void gvcf_blocks_rule(const std::vector<GvcfRec> &recs, const uint16_t *dp, const uint8_t *ref, int64_t n, int64_t first_pos, bool bp,
                             std::vector<c3_gvcf_block> &out) {
    int64_t s = -1;
    uint32_t cur_bin = 0, cur_gt = 0;
    int cur_min = 0, cur_max = 0, cur_gq = 0;
    uint8_t cur_ref = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t m = recs[i].meta;
        const uint32_t bin = gvcf_binned(m), gt = m & kGvcfValid;
        const int d = dp[i], gq = (int)gvcf_gq(m);
        bool brk, set_ref = true;
        if (s < 0) brk = true;
        else if (bin != cur_bin || gt != cur_gt) brk = true;
        else if (ref[i] != cur_ref && (ref[i] == 'N' || cur_ref == 'N')) brk = true;
        else {
            set_ref = false;
            if (d < cur_min) brk = (uint32_t)cur_max > gvcf_f((uint32_t)d);
            else if (d > cur_max) brk = !((uint32_t)d <= gvcf_f((uint32_t)cur_min));
            else brk = false;
        }
        if (brk) {
            if (s >= 0) gvcf_write_block(recs, dp, s, i - 1, first_pos, cur_min, cur_max, cur_gq, bp, out);
            s = i, cur_bin = bin, cur_gt = gt, cur_min = cur_max = d, cur_gq = gq;
            if (set_ref) cur_ref = ref[i];
        } else {
            cur_min = std::min(cur_min, d), cur_max = std::max(cur_max, d), cur_gq = std::min(cur_gq, gq);
        }
    }
    if (s >= 0) gvcf_write_block(recs, dp, s, n - 1, first_pos, cur_min, cur_max, cur_gq, bp, out);
}

template <typename T>
static int gvcf_host_records(GvcfTable &tab, const T *n_ref, const T *n_total, const uint8_t *ref, int64_t n, std::vector<GvcfRec> &recs,
                             std::vector<uint16_t> &dp) {
    recs.resize((size_t)n), dp.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        if (const char *e = gvcf_count_error((int64_t)n_ref[i], (int64_t)n_total[i]))
            return fail("gvcf: site %lld has %s (n_ref %lld, n_total %lld)", (long long)i, e, (long long)n_ref[i], (long long)n_total[i]);
    for (int64_t i = 0; i < n; ++i) {
        recs[i] = gvcf_apply_ref(tab.get((int64_t)n_ref[i], (int64_t)n_total[i]), ref[i]);
        dp[i] = (uint16_t)n_total[i];
    }
    return 0;
}

static int gvcf_check_config(const c3_gvcf_config *cfg) {
    if (!cfg) return fail("gvcf: null config");
    if (!(cfg->base_err > 0.0 && cfg->base_err < 1.0)) return fail("gvcf: base_err %g outside (0, 1)", cfg->base_err);
    if (cfg->gq_bin_size < 1 || cfg->gq_bin_size > kGvcfMaxGq) return fail("gvcf: gq_bin_size %d outside 1 .. %d", cfg->gq_bin_size, kGvcfMaxGq);
    return 0;
}

// the caller's buffer protocol: the count always, the records up to max_blocks, C3_GVCF_MORE when they do not fit
static int gvcf_deliver(const std::vector<c3_gvcf_block> &blocks, c3_gvcf_block *out, int64_t max_blocks, int64_t *n_out) {
    *n_out = (int64_t)blocks.size();
    const int64_t k = std::min<int64_t>((int64_t)blocks.size(), max_blocks);
    if (k > 0) memcpy(out, blocks.data(), (size_t)k * sizeof(c3_gvcf_block));
    return (int64_t)blocks.size() > max_blocks ? C3_GVCF_MORE : 0;
}

// ------------------------------------------------------------------------------------------ the kernels
#define C3_GVCF_TEXT __attribute__((section(".c3_gvcf_text")))  // behind `.c3_occlude_text`: no other kernel moves

struct GvcfParams {
    int64_t n;                 // sites
    // inputs
    const void *in_ref, *in_total;  // counts form: [n] int32 | int64
    const void *region;        // region form: [n_cols][18] int32 | int64
    const int64_t *major;      // [n_cols]
    int64_t n_cols, first_major;
    int in64;
    const uint8_t *ref;        // [n] reference bytes
    const GvcfRec *table;      // rows 0 .. table_depth
    const uint32_t *deep_key;  // [n_deep] the distinct packed counts deeper than the table, ascending, or nullptr
    const GvcfRec *deep;       // [n_deep] the host's records of those pairs
    int n_deep;
    int table_depth, bp;
    int64_t first_pos;
    // per site
    uint32_t *cnt;             // [n] n_ref | n_total << 16 (kGvcfBadCount: a refused count)
    GvcfRec *rec;              // [n]
    uint64_t *tree;            // levels 0 .. levels - 1, level k at lvl_off[k] with lvl_cnt[k] nodes
    int64_t lvl_off[kGvcfMaxLevels], lvl_cnt[kGvcfMaxLevels];
    int levels;
    int32_t *next;             // [n] e(s)
    uint32_t *ext;             // [n] min dp | max dp << 16 of [s, e(s))
    uint8_t *bgq;              // [n] min gq of [s, e(s))
    int32_t *last1, *last2;    // [n] last chain element of s's tile / group
    uint8_t *emit;             // [n] 1: a record starts here; 3: an item of a block written item by item
    // per tile / group
    uint32_t *tile_max;        // [tiles]
    int32_t *entry1, *cover1;  // [tiles] first chain element of the tile (-1: none), the block start in front of it
    int32_t *entry2, *cover2;  // [groups]
    uint32_t *tile_n, *tile_base;  // [tiles] records of the tile, records in front of it; tile_base[tiles] = all
    int64_t tiles, groups;
    c3_gvcf_block *out;
    int64_t out_cap;
};

// a tree node: min dp (16) | max dp (16) | min gq (8) | hard break inside (bit 40); all ones: no such node
constexpr uint64_t kGvcfHard = 1ull << 40, kGvcfAbsent = ~0ull;
__host__ __device__ __forceinline__ uint64_t gvcf_node(uint32_t mn, uint32_t mx, uint32_t gq, bool hard) {
    return (uint64_t)mn | (uint64_t)mx << 16 | (uint64_t)gq << 32 | (hard ? kGvcfHard : 0ull);
}
__host__ __device__ __forceinline__ uint64_t gvcf_merge(uint64_t a, uint64_t b) {
    if (a == kGvcfAbsent) return kGvcfAbsent;
    if (b == kGvcfAbsent) return a | kGvcfHard;  // a range that runs past the last site ends there: the region's end is a hard break
    const uint32_t mn = min((uint32_t)(a & 0xffff), (uint32_t)(b & 0xffff)), mx = max((uint32_t)(a >> 16 & 0xffff), (uint32_t)(b >> 16 & 0xffff));
    const uint32_t gq = min((uint32_t)(a >> 32 & 0xff), (uint32_t)(b >> 32 & 0xff));
    return gvcf_node(mn, mx, gq, ((a | b) & kGvcfHard) != 0);
}

constexpr uint32_t kGvcfBadCount = 0x0000ffffu;  // n_ref 65535 of n_total 0: no site has it (65535 / 65535 is all ones: a valid pair)
__device__ __forceinline__ uint32_t gvcf_pack_counts(int64_t nr, int64_t nt) {
    if (nr < 0 || nt < 0 || nr > nt || nt > kGvcfMaxDepth) return kGvcfBadCount;
    return (uint32_t)nr | (uint32_t)nt << 16;
}

C3_GVCF_TEXT __global__ __launch_bounds__(256) void gvcf_counts_kernel(GvcfParams p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int64_t nr = p.in64 ? ((const int64_t *)p.in_ref)[i] : (int64_t)((const int32_t *)p.in_ref)[i];
    const int64_t nt = p.in64 ? ((const int64_t *)p.in_total)[i] : (int64_t)((const int32_t *)p.in_total)[i];
    p.cnt[i] = gvcf_pack_counts(nr, nt);
}

// one thread per column (cnt was set to zero in front: a site without a column has 0 / 0; major is strictly increasing, checked by the
// host: no two columns write one site).  src/clair3_pileup.c:355-371 undone: channels 0 .. 3 / 9 .. 12 are A C G T forward / reverse with
// the reference base's pair replaced by minus the strand sums; 4 + 13 the insertions, 6 + 15 the deletions (:317-344)
template <typename T>
C3_GVCF_TEXT __global__ __launch_bounds__(256) void gvcf_region_kernel(GvcfParams p) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= p.n_cols) return;
    const int64_t site = p.major[c] - p.first_major;
    if (site < 0 || site >= p.n) return;
    const T *m = (const T *)p.region + c * 18;
    const uint8_t b = p.ref[site] & 0xdf;  // upper_base
    const int r = b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 0;  // base2index
    int64_t fwd_ref = 0, rev_ref = 0, alt = 0, all_alt = 0;  // the reference base's counts: the strand sums minus the other three bases'
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t f = (int64_t)m[k], v = (int64_t)m[9 + k];
        fwd_ref -= f, rev_ref -= v;  // (minus the negated strand sum at k == r, minus the count elsewhere)
        if (k == r) continue;
        bad |= f < 0 || v < 0;
        if (f + v > alt) alt = f + v, all_alt += alt;  // the reference's running-maximum sum (:360-366), not the plain sum
    }
    const int64_t n_ref = fwd_ref + rev_ref, del = (int64_t)m[6] + (int64_t)m[15], ins = (int64_t)m[4] + (int64_t)m[13];
    bad |= fwd_ref < 0 || rev_ref < 0 || del < 0 || ins < 0;
    p.cnt[site] = bad ? kGvcfBadCount : gvcf_pack_counts(n_ref, n_ref + all_alt + del + ins);
}

C3_GVCF_TEXT __global__ __launch_bounds__(kGvcfTile) void gvcf_max_kernel(GvcfParams p) {
    __shared__ uint32_t wave_max[kGvcfTile / 64];
    const int64_t i = (int64_t)blockIdx.x * kGvcfTile + threadIdx.x;
    uint32_t v = 0;
    if (i < p.n) {
        const uint32_t c = p.cnt[i];
        v = c == kGvcfBadCount ? 0xffffffffu : c >> 16;  // (a refused count outlasts the maximum)
    }
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_down(v, off, 64));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kGvcfTile / 64; ++w) s = max(s, wave_max[w]);
        p.tile_max[blockIdx.x] = s;
    }
}

__device__ __forceinline__ GvcfRec gvcf_site_record(const GvcfParams &p, int64_t i) {
    const uint32_t c = p.cnt[i];
    const int64_t nr = c & 0xffff, nt = c >> 16;
    GvcfRec raw{{0, 0, 0}, 0};
    if (nt <= p.table_depth) raw = p.table[nt * (nt + 1) / 2 + nr];
    else {  // a pair deeper than the table: binary search in the call's side table (the host put every such pair of the call there)
        int lo = 0, hi = p.n_deep;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p.deep_key[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        if (lo < p.n_deep && p.deep_key[lo] == c) raw = p.deep[lo];
    }
    return gvcf_apply_ref(raw, p.ref[i]);
}

C3_GVCF_TEXT __global__ __launch_bounds__(256) void gvcf_site_kernel(GvcfParams p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const GvcfRec r = gvcf_site_record(p, i);
    const bool hard = i == 0 || gvcf_key(gvcf_site_record(p, i - 1).meta) != gvcf_key(r.meta);
    const uint32_t dp = p.cnt[i] >> 16;
    p.rec[i] = r;
    p.tree[i] = gvcf_node(dp, dp, gvcf_gq(r.meta), hard);
}

// levels from + 1 .. from + 10 out of 1024 nodes of level `from` per workgroup
C3_GVCF_TEXT __global__ __launch_bounds__(kGvcfTile) void gvcf_tree_kernel(GvcfParams p, int from) {
    __shared__ uint64_t node[kGvcfTile];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kGvcfTile + tid;
    node[tid] = j < p.lvl_cnt[from] ? p.tree[p.lvl_off[from] + j] : kGvcfAbsent;
    __syncthreads();
    for (int k = 1; k <= kGvcfTileLog && from + k < p.levels; ++k) {
        const int width = kGvcfTile >> k;  // nodes of level from + k in this workgroup; they go to node[0 .. width)
        uint64_t v = kGvcfAbsent;
        if (tid < width) v = gvcf_merge(node[2 * tid], node[2 * tid + 1]);
        __syncthreads();
        if (tid < width) {
            node[tid] = v;
            const int64_t jj = (int64_t)blockIdx.x * width + tid;
            if (v != kGvcfAbsent && jj < p.lvl_cnt[from + k]) p.tree[p.lvl_off[from + k] + jj] = v;
        }
        __syncthreads();
    }
}

// e(s): the range (s, pos) grows by whole aligned nodes, first ever larger ones, then, behind the first node that cannot be absorbed,
// ever smaller ones.  The test is monotone, so every node is looked at once: at most 2 per level up and 1 per level down
C3_GVCF_TEXT __global__ __launch_bounds__(256) void gvcf_search_kernel(GvcfParams p) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n) return;
    const uint64_t leaf = p.tree[s];
    uint32_t mn = (uint32_t)(leaf & 0xffff), mx = mn, gq = (uint32_t)(leaf >> 32 & 0xff);
    int64_t pos = s + 1;
    int k = 0;
    auto absorb = [&](int level) -> bool {
        const int64_t j = pos >> level;
        if (j >= p.lvl_cnt[level]) return false;
        const uint64_t v = p.tree[p.lvl_off[level] + j];
        if (v & kGvcfHard) return false;
        const uint32_t mn2 = min(mn, (uint32_t)(v & 0xffff)), mx2 = max(mx, (uint32_t)(v >> 16 & 0xffff));
        if (mx2 > gvcf_f(mn2)) return false;
        mn = mn2, mx = mx2, gq = min(gq, (uint32_t)(v >> 32 & 0xff));
        pos += (int64_t)1 << level;
        return true;
    };
    while (pos < p.n && absorb(k))
        if (k + 1 < p.levels && ((pos >> k) & 1) == 0) ++k;
    if (pos < p.n)
        while (k > 0) absorb(--k);
    p.next[s] = (int32_t)min(pos, p.n);
    p.ext[s] = mn | mx << 16;
    p.bgq[s] = (uint8_t)gq;
}

// last1[s]: the last element of the chain s -> e(s) -> .. inside s's tile.  j[i] = i's successor inside the tile, or i; ten doublings
C3_GVCF_TEXT __global__ __launch_bounds__(kGvcfTile) void gvcf_last_kernel(GvcfParams p) {
    __shared__ uint16_t j[kGvcfTile];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kGvcfTile, i = t0 + tid;
    const int64_t t1 = min(t0 + kGvcfTile, p.n);
    int64_t nx = i < p.n ? p.next[i] : t1;
    j[tid] = (uint16_t)(nx < t1 ? nx - t0 : tid);
    __syncthreads();
    for (int r = 0; r < kGvcfTileLog; ++r) {
        const uint16_t v = j[j[tid]];
        __syncthreads();
        j[tid] = v;
        __syncthreads();
    }
    if (i < p.n) p.last1[i] = p.last2[i] = (int32_t)(t0 + j[tid]);
}

// round r: groups of 2^r tiles pair up.  A site of a left group whose chain goes on into the right group takes the right group's answer
// for the element it arrives at; the right group's own values do not change in this round, so the update is in place
C3_GVCF_TEXT __global__ __launch_bounds__(256) void gvcf_group_kernel(GvcfParams p, int r) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int64_t g = (int64_t)kGvcfTile << r, grp = i / g;
    if (grp & 1) return;
    const int64_t x = p.next[p.last2[i]];
    if (x < p.n && x < (grp + 2) * g) p.last2[i] = p.last2[x];
}

// thread 0 walks the groups (last2), then one thread per group walks its tiles (last1): n / 262144 and 256 steps
C3_GVCF_TEXT __global__ __launch_bounds__(256) void gvcf_entry_kernel(GvcfParams p) {
    if (threadIdx.x == 0) {
        int64_t q = 0, cover = 0;
        for (int64_t g = 0; g < p.groups; ++g) {
            const int64_t g1 = min((g + 1) * kGvcfGroupSites, p.n);
            if (q < g1) {
                p.entry2[g] = (int32_t)q, p.cover2[g] = (int32_t)cover;
                cover = p.last2[q], q = p.next[cover];
            } else p.entry2[g] = -1, p.cover2[g] = (int32_t)cover;
        }
    }
    __syncthreads();  // (one workgroup: the barrier orders thread 0's stores in front of the other threads' loads)
    for (int64_t g = threadIdx.x; g < p.groups; g += 256) {
        int64_t q = p.entry2[g], cover = p.cover2[g];
        const int64_t tA = g << kGvcfGroupLog, tB = min(tA + ((int64_t)1 << kGvcfGroupLog), p.tiles);
        if (q < 0) q = p.n;
        for (int64_t t = tA; t < tB; ++t) {
            const int64_t t1 = min((t + 1) * kGvcfTile, p.n);
            if (q < t1) {
                p.entry1[t] = (int32_t)q, p.cover1[t] = (int32_t)cover;
                cover = p.last1[q], q = p.next[cover];
            } else p.entry1[t] = -1, p.cover1[t] = (int32_t)cover;
        }
    }
}

// block starts of the tile: the chain from its entry, marked by the doubled successors from the longest jump down.  Then every site's
// block start (the last mark at or in front of it, or the tile's cover) says whether the block is written item by item
C3_GVCF_TEXT __global__ __launch_bounds__(kGvcfTile) void gvcf_mark_kernel(GvcfParams p) {
    constexpr uint16_t kOut = kGvcfTile;
    __shared__ uint16_t jump[kGvcfTileLog][kGvcfTile];
    __shared__ uint8_t mark[kGvcfTile];
    __shared__ int16_t start[kGvcfTile];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kGvcfTile, i = t0 + tid;
    const int64_t t1 = min(t0 + kGvcfTile, p.n);
    const int64_t nx = i < p.n ? p.next[i] : t1;
    jump[0][tid] = nx < t1 ? (uint16_t)(nx - t0) : kOut;
    mark[tid] = 0;
    __syncthreads();
    for (int r = 1; r < kGvcfTileLog; ++r) {
        const uint16_t a = jump[r - 1][tid];
        jump[r][tid] = a == kOut ? kOut : jump[r - 1][a];
        __syncthreads();
    }
    const int64_t e = p.entry1[blockIdx.x];
    if (tid == 0 && e >= 0) mark[e - t0] = 1;
    __syncthreads();
    for (int r = kGvcfTileLog - 1; r >= 0; --r) {
        const uint16_t a = jump[r][tid];
        const bool go = mark[tid] && a != kOut;
        __syncthreads();
        if (go) mark[a] = 1;  // (several threads may write the same 1)
        __syncthreads();
    }
    start[tid] = mark[tid] ? (int16_t)tid : (int16_t)-1;
    __syncthreads();
    for (int off = 1; off < kGvcfTile; off <<= 1) {
        const int16_t v = tid >= off ? start[tid - off] : (int16_t)-1;
        __syncthreads();
        start[tid] = max(start[tid], v);
        __syncthreads();
    }
    if (i >= p.n) return;
    const int64_t first = start[tid] >= 0 ? t0 + start[tid] : (int64_t)p.cover1[blockIdx.x];
    const uint32_t fm = p.rec[first].meta;
    const bool items = (p.bp || !(fm & kGvcfValid)) && !(fm & kGvcfNotAcgt);
    p.emit[i] = items ? 3 : mark[tid] ? 1 : 0;
}

C3_GVCF_TEXT __global__ __launch_bounds__(kGvcfTile) void gvcf_count_kernel(GvcfParams p) {
    __shared__ uint32_t wave_n[kGvcfTile / 64];
    const int64_t i = (int64_t)blockIdx.x * kGvcfTile + threadIdx.x;
    const uint64_t b = __ballot(i < p.n && p.emit[i] != 0);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kGvcfTile / 64; ++w) s += wave_n[w];
        p.tile_n[blockIdx.x] = s;
    }
}

// exclusive sums of the tiles' counts in tile order, one workgroup, 1024 tiles a step; tile_base[tiles] = all
C3_GVCF_TEXT __global__ __launch_bounds__(kGvcfTile) void gvcf_scan_kernel(GvcfParams p) {
    __shared__ uint32_t a[kGvcfTile];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < p.tiles; c0 += kGvcfTile) {
        const int64_t t = c0 + tid;
        const uint32_t own = t < p.tiles ? p.tile_n[t] : 0u;
        a[tid] = own;
        __syncthreads();
        for (int off = 1; off < kGvcfTile; off <<= 1) {
            const uint32_t v = tid >= off ? a[tid - off] : 0u;
            __syncthreads();
            a[tid] += v;
            __syncthreads();
        }
        const uint32_t base = carry;
        if (t < p.tiles) p.tile_base[t] = base + a[tid] - own;
        __syncthreads();
        if (tid == kGvcfTile - 1) carry = base + a[tid];
        __syncthreads();
    }
    if (tid == 0) p.tile_base[p.tiles] = carry;
}

// record of site i goes to slot (records in front of its tile) + (in front of its wave) + (in front of its lane); slots from out_cap on
// are not written
C3_GVCF_TEXT __global__ __launch_bounds__(kGvcfTile) void gvcf_emit_kernel(GvcfParams p) {
    __shared__ uint32_t wave_n[kGvcfTile / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * kGvcfTile + tid;
    const uint8_t em = i < p.n ? p.emit[i] : 0;
    const uint64_t b = __ballot(em != 0);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!em) return;
    int64_t slot = p.tile_base[blockIdx.x];
    for (int w = 0; w < wave; ++w) slot += wave_n[w];
    slot += __popcll(b & ((1ull << lane) - 1ull));
    if (slot >= p.out_cap) return;
    const GvcfRec r = p.rec[i];
    c3_gvcf_block o;
    o.reserved = 0;
    if (em == 3) {
        const int32_t dp = (int32_t)(p.cnt[i] >> 16);
        o.pos = o.end = p.first_pos + i, o.min_dp = o.max_dp = dp, o.gq = (int32_t)gvcf_binned(r.meta);
        o.pl[0] = r.pl[0], o.pl[1] = r.pl[1], o.pl[2] = r.pl[2];
        o.ref = (uint8_t)(r.meta >> 24), o.gt = (r.meta & kGvcfValid) ? 1 : 0, o.per_site = 1, o.first_n = 0;
    } else {
        const uint32_t x = p.ext[i];
        o.pos = p.first_pos + i, o.end = p.first_pos + p.next[i] - 1, o.min_dp = (int32_t)(x & 0xffff), o.max_dp = (int32_t)(x >> 16);
        o.per_site = 0;
        if (r.meta & kGvcfNotAcgt) o.gq = 1, o.gt = 0, o.ref = 'N', o.first_n = 1, o.pl[0] = o.pl[1] = o.pl[2] = 0;
        else {
            o.gq = p.bgq[i], o.gt = (r.meta & kGvcfValid) ? 1 : 0, o.ref = (uint8_t)(r.meta >> 24), o.first_n = 0;
            o.pl[0] = r.pl[0], o.pl[1] = r.pl[1], o.pl[2] = r.pl[2];
        }
    }
    p.out[slot] = o;
}

}  // namespace c3

// ------------------------------------------------------------------------------------------ the context
struct c3_gvcf {
    int device = 0;
    c3_gvcf_config cfg{};
    hipStream_t stream = nullptr;
    c3::GvcfTable table;
    c3::GvcfRec *d_table = nullptr;
    int d_table_depth = -1;
    struct Buf {
        void *p = nullptr;
        size_t bytes = 0;
    };
    // grown on demand, never shrunk: inputs (a, b, c), per-site arrays, per-tile arrays, records
    Buf in_a, in_b, in_c, ref, cnt, rec, tree, next, ext, bgq, last1, last2, emit, deep, deep_key, tiles, out;
};

namespace c3 {

static int gvcf_grow(c3_gvcf::Buf &b, size_t bytes) {
    if (bytes <= b.bytes) return 0;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr, b.bytes = 0;
    bytes = std::max<size_t>((bytes + 255) & ~(size_t)255, 256);
    HIP_TRY(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return 0;
}

#define GVCF_LAUNCH(kernel, grid, block, ...)                                        \
    do {                                                                             \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(block), 0, g->stream, __VA_ARGS__); \
        HIP_TRY(hipGetLastError());                                                  \
    } while (0)

// everything behind the counts: p.cnt holds the sites' counts on the device
static int gvcf_run(c3_gvcf *g, GvcfParams &p, c3_gvcf_block *blocks_out, int64_t max_blocks, int64_t *n_blocks_out) {
    const int64_t n = p.n;
    p.tiles = (n + kGvcfTile - 1) / kGvcfTile, p.groups = (n + kGvcfGroupSites - 1) / kGvcfGroupSites;
    // per-tile words: tile_max | entry1 | cover1 | tile_n | tile_base (+1) | entry2 | cover2
    TRY(gvcf_grow(g->tiles, (size_t)(5 * p.tiles + 1 + 2 * p.groups) * 4));
    p.tile_max = (uint32_t *)g->tiles.p;
    p.entry1 = (int32_t *)(p.tile_max + p.tiles), p.cover1 = p.entry1 + p.tiles;
    p.tile_n = (uint32_t *)(p.cover1 + p.tiles), p.tile_base = p.tile_n + p.tiles;
    p.entry2 = (int32_t *)(p.tile_base + p.tiles + 1), p.cover2 = p.entry2 + p.groups;
    GVCF_LAUNCH(gvcf_max_kernel, p.tiles, kGvcfTile, p);
    std::vector<uint32_t> tmax((size_t)p.tiles);
    TRY(d2h_staged(tmax.data(), p.tile_max, (size_t)p.tiles * 4, g->stream));
    uint32_t mx = 0;
    for (size_t t = 0; t < tmax.size(); ++t) {
        if (tmax[t] == 0xffffffffu)
            return fail("gvcf: a site among %lld .. %lld has a refused count (negative, n_ref > n_total, or a depth above 65535)",
                        (long long)(t * kGvcfTile), (long long)std::min<int64_t>((int64_t)(t + 1) * kGvcfTile, n) - 1);
        mx = std::max(mx, tmax[t]);
    }
    // the table: rows up to the deepest site, kGvcfTableDepth at most
    const int want = (int)std::min<uint32_t>(mx, (uint32_t)kGvcfTableDepth);
    if (want > g->d_table_depth) {
        g->table.ensure(want);
        const size_t bytes = GvcfTable::index(want + 1, 0) * sizeof(GvcfRec);
        GvcfRec *d = nullptr;
        HIP_TRY(hipMalloc((void **)&d, bytes));
        if (h2d_staged(d, g->table.rows.data(), bytes, g->stream)) {
            (void)hipFree(d);
            return 1;
        }
        if (g->d_table) HIP_TRY(hipFree(g->d_table));
        g->d_table = d, g->d_table_depth = want;
    }
    p.table = g->d_table, p.table_depth = g->d_table_depth, p.deep = nullptr, p.deep_key = nullptr, p.n_deep = 0;
    if (mx > (uint32_t)kGvcfTableDepth) {
        // sites deeper than the table: the counts come back once (4 bytes a site), the host computes the record of every DISTINCT deep
        // pair and sends them as a sorted side table: what travels and what is computed grows with the distinct pairs, not with n
        std::vector<uint32_t> cnt((size_t)n);
        TRY(d2h_staged(cnt.data(), p.cnt, (size_t)n * 4, g->stream));
        std::vector<uint32_t> keys;
        for (int64_t i = 0; i < n; ++i)
            if ((cnt[i] >> 16) > (uint32_t)kGvcfTableDepth) keys.push_back(cnt[i]);
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        std::vector<GvcfRec> recs(keys.size());
        for (size_t k = 0; k < keys.size(); ++k) recs[k] = g->table.math.site(keys[k] & 0xffff, keys[k] >> 16);
        TRY(gvcf_grow(g->deep_key, keys.size() * 4));
        TRY(gvcf_grow(g->deep, keys.size() * sizeof(GvcfRec)));
        TRY(h2d_staged(g->deep_key.p, keys.data(), keys.size() * 4, g->stream));
        TRY(h2d_staged(g->deep.p, recs.data(), keys.size() * sizeof(GvcfRec), g->stream));
        p.deep_key = (const uint32_t *)g->deep_key.p, p.deep = (const GvcfRec *)g->deep.p, p.n_deep = (int)keys.size();
    }
    // the tree's levels
    p.levels = 0;
    int64_t off = 0;
    for (int64_t c = n;; c = (c + 1) / 2) {
        p.lvl_off[p.levels] = off, p.lvl_cnt[p.levels] = c, off += c, ++p.levels;
        if (c == 1) break;
    }
    TRY(gvcf_grow(g->rec, (size_t)n * sizeof(GvcfRec)));
    TRY(gvcf_grow(g->tree, (size_t)off * 8));
    TRY(gvcf_grow(g->next, (size_t)n * 4));
    TRY(gvcf_grow(g->ext, (size_t)n * 4));
    TRY(gvcf_grow(g->bgq, (size_t)n));
    TRY(gvcf_grow(g->last1, (size_t)n * 4));
    TRY(gvcf_grow(g->last2, (size_t)n * 4));
    TRY(gvcf_grow(g->emit, (size_t)n));
    p.rec = (GvcfRec *)g->rec.p, p.tree = (uint64_t *)g->tree.p, p.next = (int32_t *)g->next.p, p.ext = (uint32_t *)g->ext.p;
    p.bgq = (uint8_t *)g->bgq.p, p.last1 = (int32_t *)g->last1.p, p.last2 = (int32_t *)g->last2.p, p.emit = (uint8_t *)g->emit.p;
    p.bp = g->cfg.bp_resolution ? 1 : 0;
    const int64_t grid256 = (n + 255) / 256;
    GVCF_LAUNCH(gvcf_site_kernel, grid256, 256, p);
    for (int from = 0; from + 1 < p.levels; from += kGvcfTileLog)
        GVCF_LAUNCH(gvcf_tree_kernel, (p.lvl_cnt[from] + kGvcfTile - 1) / kGvcfTile, kGvcfTile, p, from);
    GVCF_LAUNCH(gvcf_search_kernel, grid256, 256, p);
    GVCF_LAUNCH(gvcf_last_kernel, p.tiles, kGvcfTile, p);
    for (int r = 0; r < kGvcfGroupLog && ((int64_t)kGvcfTile << r) < n; ++r) GVCF_LAUNCH(gvcf_group_kernel, grid256, 256, p, r);
    GVCF_LAUNCH(gvcf_entry_kernel, 1, 256, p);
    GVCF_LAUNCH(gvcf_mark_kernel, p.tiles, kGvcfTile, p);
    GVCF_LAUNCH(gvcf_count_kernel, p.tiles, kGvcfTile, p);
    GVCF_LAUNCH(gvcf_scan_kernel, 1, kGvcfTile, p);
    uint32_t total = 0;
    TRY(d2h_staged(&total, p.tile_base + p.tiles, 4, g->stream));
    *n_blocks_out = (int64_t)total;
    const int64_t k = std::min<int64_t>((int64_t)total, std::max<int64_t>(max_blocks, 0));
    if (k > 0) {
        TRY(gvcf_grow(g->out, (size_t)k * sizeof(c3_gvcf_block)));
        p.out = (c3_gvcf_block *)g->out.p, p.out_cap = k;
        GVCF_LAUNCH(gvcf_emit_kernel, p.tiles, kGvcfTile, p);
        TRY(d2h_staged(blocks_out, p.out, (size_t)k * sizeof(c3_gvcf_block), g->stream));
    }
    return (int64_t)total > max_blocks ? C3_GVCF_MORE : 0;
}

static int gvcf_common_checks(c3_gvcf *g, const void *ref_bytes, int64_t n_sites, int64_t first_pos, c3_gvcf_block *blocks_out,
                              int64_t max_blocks, int64_t *n_blocks_out, const char *what) {
    if (!g) return fail("%s: null context", what);
    if (!n_blocks_out) return fail("%s: null n_blocks_out", what);
    if (n_sites < 0 || max_blocks < 0) return fail("%s: a negative count", what);
    if (n_sites > 0 && !ref_bytes) return fail("%s: null reference bytes", what);
    if (max_blocks > 0 && !blocks_out) return fail("%s: null blocks_out", what);
    if (n_sites > (int64_t)INT32_MAX - kGvcfTile) return fail("%s: %lld sites in one call (at most %lld)", what, (long long)n_sites, (long long)INT32_MAX - kGvcfTile);
    if (first_pos < 0) return fail("%s: a negative first_pos", what);
    return 0;
}

}  // namespace c3

extern "C" {

int c3_gvcf_tile_sites(void) { return c3::kGvcfTile; }
int64_t c3_gvcf_top_span(void) { return c3::kGvcfGroupSites; }
int c3_gvcf_table_depth(void) { return c3::kGvcfTableDepth; }

int c3_gvcf_site(const c3_gvcf_config *cfg, int64_t n_ref, int64_t n_total, int ref_byte, int32_t *out6) {
    using namespace c3;
    TRY(gvcf_check_config(cfg));
    if (!out6) return fail("c3_gvcf_site: null output");
    if (const char *e = gvcf_count_error(n_ref, n_total)) return fail("c3_gvcf_site: %s", e);
    GvcfMath m;
    m.set(cfg->base_err, cfg->gq_bin_size);
    const GvcfRec r = gvcf_apply_ref(m.site(n_ref, n_total), (uint8_t)ref_byte);
    out6[0] = (int32_t)gvcf_gq(r.meta), out6[1] = (int32_t)gvcf_binned(r.meta), out6[2] = (r.meta & kGvcfValid) ? 1 : 0;
    out6[3] = r.pl[0], out6[4] = r.pl[1], out6[5] = r.pl[2];
    return 0;
}

int c3_gvcf_site_table(const c3_gvcf_config *cfg, int depth, int32_t *out) {
    using namespace c3;
    TRY(gvcf_check_config(cfg));
    if (!out || depth < 0 || depth > kGvcfMaxDepth) return fail("c3_gvcf_site_table: null output or a depth outside 0 .. 65535");
    GvcfMath m;
    m.set(cfg->base_err, cfg->gq_bin_size);
    for (int nt = 0; nt <= depth; ++nt)
        for (int nr = 0; nr <= nt; ++nr) {
            const GvcfRec r = m.site(nr, nt);
            int32_t *o = out + 6 * GvcfTable::index(nt, nr);
            o[0] = (int32_t)gvcf_gq(r.meta), o[1] = (int32_t)gvcf_binned(r.meta), o[2] = (r.meta & kGvcfValid) ? 1 : 0;
            o[3] = r.pl[0], o[4] = r.pl[1], o[5] = r.pl[2];
        }
    return 0;
}

int c3_gvcf_blocks_host(const c3_gvcf_config *cfg, const void *n_ref, const void *n_total, int dtype, const void *ref_bytes, int64_t n_sites,
                        int64_t first_pos, c3_gvcf_block *blocks_out, int64_t max_blocks, int64_t *n_blocks_out) {
    using namespace c3;
    TRY(gvcf_check_config(cfg));
    if (!n_blocks_out) return fail("c3_gvcf_blocks_host: null n_blocks_out");
    if (n_sites < 0 || max_blocks < 0 || first_pos < 0) return fail("c3_gvcf_blocks_host: a negative count or position");
    if (n_sites > 0 && (!n_ref || !n_total || !ref_bytes)) return fail("c3_gvcf_blocks_host: null buffer");
    if (max_blocks > 0 && !blocks_out) return fail("c3_gvcf_blocks_host: null blocks_out");
    if (dtype != C3_DTYPE_I32 && dtype != C3_DTYPE_I64) return fail("c3_gvcf_blocks_host: counts are int32 or int64");
    *n_blocks_out = 0;
    if (n_sites == 0) return 0;
    GvcfTable tab;
    tab.math.set(cfg->base_err, cfg->gq_bin_size);
    std::vector<GvcfRec> recs;
    std::vector<uint16_t> dp;
    if (dtype == C3_DTYPE_I32) TRY(gvcf_host_records(tab, (const int32_t *)n_ref, (const int32_t *)n_total, (const uint8_t *)ref_bytes, n_sites, recs, dp));
    else TRY(gvcf_host_records(tab, (const int64_t *)n_ref, (const int64_t *)n_total, (const uint8_t *)ref_bytes, n_sites, recs, dp));
    std::vector<c3_gvcf_block> blocks;
    gvcf_blocks_rule(recs, dp.data(), (const uint8_t *)ref_bytes, n_sites, first_pos, cfg->bp_resolution != 0, blocks);
    return gvcf_deliver(blocks, blocks_out, max_blocks, n_blocks_out);
}

int c3_gvcf_text(const c3_gvcf_block *blocks, int64_t n_blocks, const char *ctg_name, int64_t contig_len, int64_t first_pos, int64_t n_sites,
                 char *buf, int64_t buf_bytes, int64_t *bytes_out) {
    using namespace c3;
    if (!bytes_out || !ctg_name) return fail("c3_gvcf_text: null argument");
    if (n_blocks < 0 || buf_bytes < 0) return fail("c3_gvcf_text: a negative count");
    if (n_blocks > 0 && !blocks) return fail("c3_gvcf_text: null blocks");
    if (buf_bytes > 0 && !buf) return fail("c3_gvcf_text: null buffer");
    std::string s;
    s.reserve((size_t)n_blocks * 72 + 128);
    char line[256];
    const size_t name = strlen(ctg_name);
    auto put = [&](int64_t pos, char ref, int64_t end, bool gt, int gq, int dp, const int32_t *pl) {
        if (contig_len > 0 && end == contig_len - 1) end = contig_len;  // write_to_gvcf :614-616
        s.append(ctg_name, name);
        const int k = snprintf(line, sizeof(line), "\t%lld\t.\t%c\t<NON_REF>\t0\t.\tEND=%lld\tGT:GQ:MIN_DP:PL\t%s:%d:%d:%d,%d,%d\n", (long long)pos, ref,
                               (long long)end, gt ? "0/0" : "./.", gq, dp, pl[0], pl[1], pl[2]);
        s.append(line, (size_t)k);
    };
    bool empty = n_blocks > 0 && n_sites > 0;  // (n_sites == 0: the records as they are)
    for (int64_t i = 0; i < n_blocks && empty; ++i) empty = blocks[i].max_dp == 0;
    if (empty) {  // write_empty_pileup :392-397 (the loop of the producer never ran: CreateTensorPileupFromCffi.py:417-421, :439-440)
        const int32_t pl[3] = {0, 0, 0};
        put(std::max<int64_t>(1, first_pos), 'N', first_pos + n_sites, false, 1, 0, pl);
    } else
        for (int64_t i = 0; i < n_blocks; ++i) {
            const c3_gvcf_block &b = blocks[i];
            put(b.pos, (char)b.ref, b.end, b.gt != 0, b.gq, b.min_dp, b.pl);
        }
    *bytes_out = (int64_t)s.size();
    if ((int64_t)s.size() > buf_bytes) return C3_GVCF_MORE;
    if (!s.empty()) memcpy(buf, s.data(), s.size());
    return 0;
}

c3_gvcf *c3_gvcf_create(int device, const c3_gvcf_config *cfg) {
    using namespace c3;
    if (gvcf_check_config(cfg)) return nullptr;
    const int ndev = c3_device_count();
    if (ndev <= 0) {
        fail("c3_gvcf_create: no HIP device visible (c3_gvcf_blocks_host needs none)");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail("c3_gvcf_create: device %d out of range (%d visible)", device, ndev);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        fail("hipSetDevice(%d) failed", device);
        return nullptr;
    }
    c3_gvcf *g = new c3_gvcf();
    g->device = device, g->cfg = *cfg;
    g->table.math.set(cfg->base_err, cfg->gq_bin_size);
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
        fail("c3_gvcf_create: hipStreamCreate failed");
        delete g;
        return nullptr;
    }
    return g;
}

int c3_gvcf_destroy(c3_gvcf *g) {
    if (!g) return 0;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream), (void)hipStreamDestroy(g->stream);
    for (c3_gvcf::Buf *b : {&g->in_a, &g->in_b, &g->in_c, &g->ref, &g->cnt, &g->rec, &g->tree, &g->next, &g->ext, &g->bgq, &g->last1, &g->last2,
                            &g->emit, &g->deep, &g->deep_key, &g->tiles, &g->out})
        if (b->p) (void)hipFree(b->p);
    if (g->d_table) (void)hipFree(g->d_table);
    delete g;
    return 0;
}

int c3_gvcf_blocks_counts(c3_gvcf *g, const void *n_ref, const void *n_total, int dtype, const void *ref_bytes, int64_t n_sites, int64_t first_pos,
                          c3_gvcf_block *blocks_out, int64_t max_blocks, int64_t *n_blocks_out) {
    using namespace c3;
    TRY(gvcf_common_checks(g, ref_bytes, n_sites, first_pos, blocks_out, max_blocks, n_blocks_out, "c3_gvcf_blocks_counts"));
    if (n_sites > 0 && (!n_ref || !n_total)) return fail("c3_gvcf_blocks_counts: null counts");
    if (dtype != C3_DTYPE_I32 && dtype != C3_DTYPE_I64) return fail("c3_gvcf_blocks_counts: counts are int32 or int64");
    *n_blocks_out = 0;
    if (n_sites == 0) return 0;
    HIP_TRY(hipSetDevice(g->device));
    const size_t item = dtype == C3_DTYPE_I64 ? 8 : 4;
    TRY(gvcf_grow(g->in_a, (size_t)n_sites * item));
    TRY(gvcf_grow(g->in_b, (size_t)n_sites * item));
    TRY(gvcf_grow(g->ref, (size_t)n_sites));
    TRY(gvcf_grow(g->cnt, (size_t)n_sites * 4));
    TRY(h2d_staged(g->in_a.p, n_ref, (size_t)n_sites * item, g->stream));
    TRY(h2d_staged(g->in_b.p, n_total, (size_t)n_sites * item, g->stream));
    TRY(h2d_staged(g->ref.p, ref_bytes, (size_t)n_sites, g->stream));
    GvcfParams p{};
    p.n = n_sites, p.in_ref = g->in_a.p, p.in_total = g->in_b.p, p.in64 = dtype == C3_DTYPE_I64, p.ref = (const uint8_t *)g->ref.p;
    p.cnt = (uint32_t *)g->cnt.p, p.first_pos = first_pos;
    GVCF_LAUNCH(gvcf_counts_kernel, (n_sites + 255) / 256, 256, p);
    return gvcf_run(g, p, blocks_out, max_blocks, n_blocks_out);
}

int c3_gvcf_blocks_region(c3_gvcf *g, const void *region_host, int x_dtype, int64_t n_cols, const int64_t *major_host, const void *ref_bytes,
                          int64_t first_major, int64_t n_sites, int64_t first_pos, c3_gvcf_block *blocks_out, int64_t max_blocks,
                          int64_t *n_blocks_out) {
    using namespace c3;
    TRY(gvcf_common_checks(g, ref_bytes, n_sites, first_pos, blocks_out, max_blocks, n_blocks_out, "c3_gvcf_blocks_region"));
    if (n_cols < 0) return fail("c3_gvcf_blocks_region: a negative column count");
    if (n_cols > 0 && (!region_host || !major_host)) return fail("c3_gvcf_blocks_region: null region or major");
    if (x_dtype != C3_DTYPE_I32 && x_dtype != C3_DTYPE_I64) return fail("c3_gvcf_blocks_region: the region is int32 or int64 (18 counts a column)");
    for (int64_t c = 1; c < n_cols; ++c)
        if (major_host[c] <= major_host[c - 1]) return fail("c3_gvcf_blocks_region: major is not strictly increasing at column %lld", (long long)c);
    *n_blocks_out = 0;
    if (n_sites == 0) return 0;
    HIP_TRY(hipSetDevice(g->device));
    const size_t item = x_dtype == C3_DTYPE_I64 ? 8 : 4;
    TRY(gvcf_grow(g->in_a, (size_t)n_cols * 18 * item));
    TRY(gvcf_grow(g->in_c, (size_t)n_cols * 8));
    TRY(gvcf_grow(g->ref, (size_t)n_sites));
    TRY(gvcf_grow(g->cnt, (size_t)n_sites * 4));
    if (n_cols > 0) {
        TRY(h2d_staged(g->in_a.p, region_host, (size_t)n_cols * 18 * item, g->stream));
        TRY(h2d_staged(g->in_c.p, major_host, (size_t)n_cols * 8, g->stream));
    }
    TRY(h2d_staged(g->ref.p, ref_bytes, (size_t)n_sites, g->stream));
    HIP_TRY(hipMemsetAsync(g->cnt.p, 0, (size_t)n_sites * 4, g->stream));
    GvcfParams p{};
    p.n = n_sites, p.region = g->in_a.p, p.major = (const int64_t *)g->in_c.p, p.n_cols = n_cols, p.first_major = first_major;
    p.in64 = x_dtype == C3_DTYPE_I64, p.ref = (const uint8_t *)g->ref.p, p.cnt = (uint32_t *)g->cnt.p, p.first_pos = first_pos;
    if (n_cols > 0) {
        if (p.in64) GVCF_LAUNCH(gvcf_region_kernel<int64_t>, (n_cols + 255) / 256, 256, p);
        else GVCF_LAUNCH(gvcf_region_kernel<int32_t>, (n_cols + 255) / 256, 256, p);
    }
    return gvcf_run(g, p, blocks_out, max_blocks, n_blocks_out);
}

}  // extern "C"
