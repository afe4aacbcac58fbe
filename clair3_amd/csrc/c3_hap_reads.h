// c3_hap_reads.h -- haplotagging the reads on the device: haplotag_read (src/clair3_full_alignment_dwell.c:262-422) over a c3_read_set and the
// c3_phased_variants of its contig.  The rule, its quirks and the host form: c3_hap_rule.h; hap_pair_allele / hap_vote / hap_tag of that
// header are called from the kernels below as they are from the host form.
//
// The host checks the input in one pass (hap_check: the reads' ends, per read two binary searches over the variants' positions for its
// pairs, the prefix sum of the pair counts, the coverage of every context) and stages it.  The launches, on the context's stream:
//   pileup_ops_kernel   (c3_pileup.h, shared, not copied) the per-read op table.  In a chained call it is the one launch the window kernels
//                       use too
//   hap_pair_kernel     one lane per (read, variant) pair: its read by binary search in the pair offsets, the owning op by binary search in
//                       the read's op table (the first I op at the variant's place in front of the op behind it), the two context walks,
//                       both edit distances in one pass over the query.  The DP rows run along the ref / alt string (at most 21 bytes) and
//                       live in registers as fully unrolled arrays; the query is streamed from the packed nibbles and may be of any length.
//                       One int8 allele per pair
//   hap_vote_kernel     one wave per read.  Steps of 64 pairs: lane l takes pair i = base + l, sums the votes of every pair of the read with
//                       its phase set and learns whether an earlier voting pair has that set (then it is not the set's leader); the leaders'
//                       sums go into the wave's max / min.  Integer sums: any order gives the same bytes.  No table, so no capacity: a read
//                       over hundreds of variants takes more steps.  Writes tags[r]
// No atomics, no device printf or assert.
#pragma once
#include <hip/hip_runtime.h>
#include "c3_fa_reads.h"

namespace c3 {

#define C3_HAP_TEXT __attribute__((section(".c3_hap_text")))  // behind `.c3_fa_text`: no other kernel moves

constexpr int kHapBlock = 256, kHapVoteChunk = 64;

struct HapParams {
    HapView h;
    int8_t *alleles;  // [n_pairs]
    uint8_t *tags;    // [n_reads]
};

C3_HAP_TEXT __global__ __launch_bounds__(kHapBlock) void hap_pair_kernel(HapParams p) {
    const int64_t i = (int64_t)blockIdx.x * kHapBlock + threadIdx.x;
    if (i >= p.h.n_pairs) return;
    int64_t a = 0, b = p.h.n_reads;  // the last read whose first pair is at or in front of i (reads without pairs share their offset with
    while (b - a > 1) {              // the read behind them: the last of such a run is the one that has pairs)
        const int64_t m = (a + b) >> 1;
        if (p.h.pair_first[m] <= i) a = m;
        else b = m;
    }
    p.alleles[i] = (int8_t)hap_pair_allele(p.h, a, p.h.var_first[a] + (i - p.h.pair_first[a]));
}

C3_HAP_TEXT __global__ __launch_bounds__(kHapBlock) void hap_vote_kernel(HapParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kHapBlock / 64) + (threadIdx.x >> 6);
    if (r >= p.h.n_reads) return;  // (wave-uniform)
    const HapView &h = p.h;
    const int64_t p0 = h.pair_first[r], n = h.pair_first[r + 1] - p0, v0 = h.var_first[r];
    int32_t max_v = 0, min_v = 0;
    bool any = false;
    for (int64_t base = 0; base < n; base += kHapVoteChunk) {  // (n is the same in every lane)
        const int64_t i = base + lane;
        const int mine = i < n ? (int)p.alleles[p0 + i] : 0;
        if (mine != 0) {
            const int32_t set = h.vps[v0 + i];
            int32_t sum = 0;
            bool leader = true;
            for (int64_t j = 0; j < n; ++j) {
                const int a = (int)p.alleles[p0 + j];
                if (a != 0 && h.vps[v0 + j] == set) {
                    sum += hap_vote(h, v0 + j, a);
                    if (j < i) leader = false;
                }
            }
            if (leader) max_v = sum > max_v ? sum : max_v, min_v = sum < min_v ? sum : min_v;
            any = true;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t a = __shfl_xor(max_v, off, 64), b = __shfl_xor(min_v, off, 64);
        max_v = a > max_v ? a : max_v, min_v = b < min_v ? b : min_v;
    }
    const bool some = __ballot(any) != 0;
    if (lane == 0) p.tags[r] = (uint8_t)hap_tag(some, max_v, min_v);
}

// ------------------------------------------------------------------------------------------ staging and launches
// the variants, the per-read pair ranges and the reference bytes the contexts read: grown and queued on the context's stream
static int hap_stage(c3_fa_reads_ctx *g, const HapJob &job, int64_t n_reads) {
    const HapTables &t = *job.t;
    const int64_t nv = job.vars->n;
    hipStream_t st = g->stream;
    HIP_TRY(hipEventRecord(g->hev[0], st));
    TRY(pileup_grow(g->tags, (size_t)n_reads));
    TRY(pileup_grow(g->alleles, (size_t)t.n_pairs));
    TRY(pileup_grow(g->pair_first, (size_t)(n_reads + 1) * 8));
    TRY(pileup_grow(g->var_first, (size_t)n_reads * 8));
    TRY(h2d_staged(g->pair_first.p, t.pair_first.data(), (size_t)(n_reads + 1) * 8, st));
    if (n_reads) TRY(h2d_staged(g->var_first.p, t.var_first.data(), (size_t)n_reads * 8, st));
    if (t.n_pairs == 0) return 0;  // (no pair reads a variant or a reference byte)
    // the variants and reference bytes under the reads that have pairs
    int64_t v_lo = nv, v_hi = 0;
    for (int64_t r = 0; r < n_reads; ++r)
        if (t.pair_first[(size_t)r + 1] > t.pair_first[(size_t)r])
            v_lo = std::min(v_lo, t.var_first[(size_t)r]), v_hi = std::max(v_hi, t.var_first[(size_t)r] + t.pair_first[(size_t)r + 1] - t.pair_first[(size_t)r]);
    const int64_t ref_lo = job.vars->pos[v_lo] - kHapOverhang, ref_n = job.vars->pos[v_hi - 1] + kHapOverhang + 1 - ref_lo;
    g->hap_ref_first = ref_lo;
    struct Up { c3_pileup::Buf *b; const void *src; size_t bytes; };
    const Up ups[] = {{&g->vpos, job.vars->pos, (size_t)nv * 8}, {&g->valt, job.vars->alt_base, (size_t)nv}, {&g->vgt, job.vars->genotype, (size_t)nv},
                      {&g->vps, job.vars->phase_set, (size_t)nv * 4}, {&g->hap_ref, job.ref + (ref_lo - job.ref_first), (size_t)ref_n}};
    for (const Up &u : ups) TRY(pileup_grow(*u.b, u.bytes));
    for (const Up &u : ups) TRY(h2d_staged(u.b->p, u.src, u.bytes, st));
    return 0;
}

// behind the op table of the same reads (g->cfirst, g->sfirst, g->cigar, g->seq, g->op_rpos, g->op_q hold this call's read set)
static int hap_launch(c3_fa_reads_ctx *g, const HapJob &job, int64_t n_reads) {
    const HapTables &t = *job.t;
    hipStream_t st = g->stream;
    HapParams p{};
    p.h.n_reads = n_reads, p.h.n_pairs = t.n_pairs, p.h.cigar_first = (const int64_t *)g->cfirst.p, p.h.seq_first = (const int64_t *)g->sfirst.p;
    p.h.cigar = (const uint32_t *)g->cigar.p, p.h.seq = (const uint8_t *)g->seq.p;
    p.h.op_rpos = (const int64_t *)g->op_rpos.p, p.h.op_q = (const int32_t *)g->op_q.p, p.h.ref = (const uint8_t *)g->hap_ref.p;
    p.h.vpos = (const int64_t *)g->vpos.p, p.h.valt = (const uint8_t *)g->valt.p, p.h.vgt = (const uint8_t *)g->vgt.p, p.h.vps = (const int32_t *)g->vps.p;
    p.h.pair_first = (const int64_t *)g->pair_first.p, p.h.var_first = (const int64_t *)g->var_first.p, p.h.ref_first = g->hap_ref_first;
    p.alleles = (int8_t *)g->alleles.p, p.tags = (uint8_t *)g->tags.p;
    HIP_TRY(hipEventRecord(g->hev[2], st));
    if (t.n_pairs > 0) PILEUP_LAUNCH(hap_pair_kernel, (t.n_pairs + kHapBlock - 1) / kHapBlock, kHapBlock, p);
    HIP_TRY(hipEventRecord(g->hev[3], st));
    if (n_reads > 0) PILEUP_LAUNCH(hap_vote_kernel, (n_reads + kHapBlock / 64 - 1) / (kHapBlock / 64), kHapBlock, p);
    HIP_TRY(hipEventRecord(g->hev[4], st));
    g->tags_on_host = false, g->hap_counted = false, g->hap_reads = n_reads, g->hap_pairs = t.n_pairs;
    g->tagged.pair_first = t.pair_first;
    return 0;
}

// the tags of a device call into g->tagged.hap
static int hap_fetch_tags(c3_fa_reads_ctx *g) {
    g->tagged.hap.resize((size_t)g->hap_reads);
    if (g->tags_on_host || g->hap_reads == 0) return 0;
    HIP_TRY(hipSetDevice(g->device));
    return d2h_staged(g->tagged.hap.data(), g->tags.p, (size_t)g->hap_reads, g->stream);
}

static void hap_reset(c3_fa_reads_ctx *g) {  // whatever happens next, a refusal included, the context holds no stale tags
    g->tagged.clear(), g->tags_on_host = true, g->hap_counted = true, g->hap_reads = g->hap_pairs = 0, g->hap_stats = c3_haplotag_counters{};
}

static void hap_count(c3_fa_reads_ctx *g) {
    c3_haplotag_counters &s = g->hap_stats;
    s.reads_hap[0] = s.reads_hap[1] = s.reads_hap[2] = 0, s.pairs_allele0 = 0;
    for (uint8_t t : g->tagged.hap) ++s.reads_hap[t < 3 ? t : 0];
    for (int8_t a : g->tagged.alleles) s.pairs_allele0 += a == 0;
    s.pairs_realigned = g->hap_pairs;
    g->hap_counted = true;
}

static int hap_held_on_host(c3_fa_reads_ctx *g, const HapView &h, const HapTables &t) {
    hap_rule_host(h, g->tagged);
    g->tags_on_host = true, g->hap_reads = h.n_reads, g->hap_pairs = t.n_pairs, g->hap_stats.on_host = 1;
    hap_count(g);
    return 0;
}

// the stand-alone device call: the read arrays the op table and the pair kernel read, the op table, the two kernels
static int hap_device(c3_fa_reads_ctx *g, const c3_read_set *rs, const HapJob &job) {
    HIP_TRY(hipSetDevice(g->device));
    const HapTables &t = *job.t;
    const int64_t nr = rs->n_reads, n_ops = t.n_ops, seq_bytes = t.sfirst[(size_t)nr];
    hipStream_t st = g->stream;
    if (nr == 0) {
        g->tags_on_host = false, g->hap_counted = false, g->hap_reads = g->hap_pairs = 0, g->tagged.pair_first = t.pair_first;
        return 0;
    }
    // (the op table kernel reads flag, mapq and min_mq for a field nothing here uses: a read set without flags is staged with zeros)
    std::vector<uint16_t> no_flag((size_t)nr, 0);
    struct Up { c3_pileup::Buf *b; const void *src; size_t bytes; };
    const Up ups[] = {{&g->pos, rs->pos, (size_t)nr * 8}, {&g->flag, rs->flag ? (const void *)rs->flag : (const void *)no_flag.data(), (size_t)nr * 2},
                      {&g->mapq, rs->mapq, (size_t)nr}, {&g->cfirst, t.cfirst.data(), (size_t)(nr + 1) * 8}, {&g->sfirst, t.sfirst.data(), (size_t)(nr + 1) * 8},
                      {&g->cigar, rs->cigar ? rs->cigar + t.c_base : nullptr, (size_t)n_ops * 4}, {&g->seq, rs->seq ? rs->seq + t.s_base : nullptr, (size_t)seq_bytes}};
    for (const Up &u : ups) TRY(pileup_grow(*u.b, u.bytes));
    TRY(pileup_grow(g->op_rpos, (size_t)n_ops * 8));
    TRY(pileup_grow(g->op_q, (size_t)n_ops * 4));
    TRY(pileup_grow(g->op_read, (size_t)n_ops * 4));
    TRY(hap_stage(g, job, nr));  // (records hev[0] first)
    for (const Up &u : ups)
        if (u.bytes) TRY(h2d_staged(u.b->p, u.src, u.bytes, st));
    HIP_TRY(hipEventRecord(g->hev[1], st));
    PileupParams pp{};
    pp.n_reads = nr, pp.n_ops = n_ops, pp.pos = (const int64_t *)g->pos.p, pp.cigar_first = (const int64_t *)g->cfirst.p, pp.flag = (const uint16_t *)g->flag.p;
    pp.mapq = (const uint8_t *)g->mapq.p, pp.cigar = (const uint32_t *)g->cigar.p, pp.op_rpos = (int64_t *)g->op_rpos.p, pp.op_q = (int32_t *)g->op_q.p;
    pp.op_read = (int32_t *)g->op_read.p;
    PILEUP_LAUNCH(pileup_ops_kernel, (nr + 3) / 4, 256, pp);
    TRY(hap_launch(g, job, nr));
    HIP_TRY(hipStreamSynchronize(st));
    const int span[4][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}};  // staging in, op table, pairs, votes
    for (int k = 0; k < 4; ++k) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, g->hev[span[k][0]], g->hev[span[k][1]]));
        g->hap_stats.kernel_ms[k] = ms;
    }
    return 0;
}

static int hap_entry(c3_fa_reads_ctx *g, const c3_read_set *rs, const c3_phased_variants *vs, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                     const c3_haplotag_config *cfg, bool device, const char *what) {
    if (!g) return fail("%s: null context", what);
    hap_reset(g);
    if (device && g->device < 0) return fail("%s: this context was created without a device (c3_fa_haplotag_host needs none)", what);
    HapTables t;
    TRY(hap_check(rs, vs, ref_bytes, ref_first, ref_len, cfg, t));
    g->hap_stats.reads_low_mapq = t.n_low;
    if (!device) return hap_held_on_host(g, hap_view(rs, vs, t, (const uint8_t *)ref_bytes, ref_first), t);
    const HapJob job{vs, &t, (const uint8_t *)ref_bytes, ref_first};
    return hap_device(g, rs, job);
}

// tag, then build the windows.  The window rule's checks see extras whose haplotype is the tag array of the context.  dwell: with the
// dwell channel from `moves` (c3_dwell.h)
static int fa_phased_entry(c3_fa_reads_ctx *g, const c3_read_set *rs, const c3_read_extras *ex, const c3_phased_variants *vs, const int64_t *centres,
                           int64_t n_cand, const void *ref_bytes, int64_t ref_first, int64_t ref_len, const c3_fa_config *cfg,
                           const c3_haplotag_config *hcfg, bool device, const char *what, const c3_read_moves *moves = nullptr, bool dwell = false) {
    if (!g) return fail("%s: null context", what);
    fa_reset(g);
    hap_reset(g);
    if (device && g->device < 0) return fail("%s: this context was created without a device (the _host entry needs none)", what);
    if (!ex) return fail("%s: null extras", what);
    HapTables ht;
    TRY(hap_check(rs, vs, ref_bytes, ref_first, ref_len, hcfg, ht));
    g->tagged.hap.assign((size_t)rs->n_reads, 0);
    static const uint8_t none = 0;
    c3_read_extras with = *ex;
    with.haplotype = rs->n_reads ? g->tagged.hap.data() : &none;
    FaTables t;
    const int rc = fa_check(rs, &with, centres, n_cand, ref_bytes, ref_first, ref_len, cfg, t);
    if (rc) return hap_reset(g), rc;
    DwTables d;
    if (dwell && fa_dwell_check(moves, t, rs->n_reads, d, what)) return hap_reset(g), 1;
    const DwJob dwj{moves, &d};
    const DwJob *dw = dwell ? &dwj : nullptr;
    g->host.channels = dwell ? kDwChannels : kFaChannels;
    g->stats.reads_kept = t.n_kept, g->stats.reads_dropped = t.n_dropped, g->host.matrix_depth = cfg->matrix_depth;
    g->hap_stats.reads_low_mapq = ht.n_low;
    const HapJob job{vs, &ht, (const uint8_t *)ref_bytes, ref_first};
    if (!device || n_cand == 0) {  // (no candidates: nothing of the window step is queued; the tags are computed all the same)
        if (device) TRY(hap_device(g, rs, job));
        else TRY(hap_held_on_host(g, hap_view(rs, vs, ht, (const uint8_t *)ref_bytes, ref_first), ht));
        if (n_cand == 0) return 0;
        with.haplotype = rs->n_reads ? g->tagged.hap.data() : &none;  // (hap_rule_host has made a new array)
        return fa_held_on_host(g, rs, t, fa_view(rs, &with, t, (const uint8_t *)ref_bytes, ref_first), centres, n_cand, *cfg, dw);
    }
    const int rc2 = fa_device(g, rs, t, fa_view(rs, &with, t, (const uint8_t *)ref_bytes, ref_first), centres, n_cand, *cfg, &job, dw);
    if (rc2) return rc2;
    const int span[3][2] = {{0, 1}, {2, 3}, {3, 4}};  // staging in (with the window step's), pairs, votes; the op table is the window step's
    const int slot[3] = {0, 2, 3};
    for (int k = 0; k < 3; ++k) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, k == 0 ? g->ev[0] : g->hev[span[k][0]], k == 0 ? g->ev[1] : g->hev[span[k][1]]));
        g->hap_stats.kernel_ms[slot[k]] = ms;
    }
    g->hap_stats.kernel_ms[1] = g->stats.kernel_ms[1];
    return 0;
}

}  // namespace c3

extern "C" {

int c3_fa_haplotag(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_phased_variants *variants, const void *ref_bytes, int64_t ref_first,
                   int64_t ref_len, const c3_haplotag_config *cfg) {
    return c3::hap_entry(g, reads, variants, ref_bytes, ref_first, ref_len, cfg, true, "c3_fa_haplotag");
}

int c3_fa_haplotag_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_phased_variants *variants, const void *ref_bytes,
                        int64_t ref_first, int64_t ref_len, const c3_haplotag_config *cfg) {
    return c3::hap_entry(g, reads, variants, ref_bytes, ref_first, ref_len, cfg, false, "c3_fa_haplotag_host");
}

int c3_fa_haplotag_sizes(c3_fa_reads_ctx *g, int64_t *n_reads, int64_t *n_pairs) {
    if (!g) return fail("c3_fa_haplotag_sizes: null context");
    if (n_reads) *n_reads = g->hap_reads;
    if (n_pairs) *n_pairs = g->hap_pairs;
    return 0;
}

int c3_fa_haplotag_result(c3_fa_reads_ctx *g, uint8_t *hap, int8_t *alleles, int64_t *pair_first) {
    using namespace c3;
    if (!g) return fail("c3_fa_haplotag_result: null context");
    if (pair_first && !g->tagged.pair_first.empty()) memcpy(pair_first, g->tagged.pair_first.data(), g->tagged.pair_first.size() * 8);
    if (g->tags_on_host) {
        if (hap && g->hap_reads) memcpy(hap, g->tagged.hap.data(), (size_t)g->hap_reads);
        if (alleles && g->hap_pairs) memcpy(alleles, g->tagged.alleles.data(), (size_t)g->hap_pairs);
        return 0;
    }
    HIP_TRY(hipSetDevice(g->device));
    if (hap && g->hap_reads) TRY(d2h_staged(hap, g->tags.p, (size_t)g->hap_reads, g->stream));
    if (alleles && g->hap_pairs) TRY(d2h_staged(alleles, g->alleles.p, (size_t)g->hap_pairs, g->stream));
    return 0;
}

int c3_fa_haplotag_stats(c3_fa_reads_ctx *g, c3_haplotag_counters *out) {
    using namespace c3;
    if (!g || !out) return fail("c3_fa_haplotag_stats: null argument");
    if (!g->hap_counted) {  // a device call: counted from one fetch, when asked for
        TRY(hap_fetch_tags(g));
        g->tagged.alleles.resize((size_t)g->hap_pairs);
        if (g->hap_pairs) TRY(d2h_staged(g->tagged.alleles.data(), g->alleles.p, (size_t)g->hap_pairs, g->stream));
        hap_count(g);
    }
    *out = g->hap_stats;
    return 0;
}

int c3_fa_haplotag_shape(int32_t *pair_block, int32_t *vote_chunk) {
    if (pair_block) *pair_block = c3::kHapBlock;
    if (vote_chunk) *vote_chunk = c3::kHapVoteChunk;
    return 0;
}

int c3_fa_reads_phased(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_phased_variants *variants,
                       const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                       const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg) {
    return c3::fa_phased_entry(g, reads, extras, variants, centres, n_cand, ref_bytes, ref_first, ref_len, fa_cfg, hap_cfg, true, "c3_fa_reads_phased");
}

int c3_fa_reads_phased_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_phased_variants *variants,
                            const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                            const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg) {
    return c3::fa_phased_entry(g, reads, extras, variants, centres, n_cand, ref_bytes, ref_first, ref_len, fa_cfg, hap_cfg, false,
                               "c3_fa_reads_phased_host");
}

}  // extern "C"
