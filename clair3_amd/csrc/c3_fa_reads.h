// c3_fa_reads.h -- full alignment from reads on the device: the candidate windows of calculate_clair3_full_alignment
// (src/clair3_full_alignment_dwell.c:437-1054) from a c3_read_set and its c3_read_extras, as occupied rows and row counts.  The rule, its
// deviations and the host form: c3_fa_rule.h; fa_bounds / fa_pos / fa_ins_equal / fa_af / fa_ch6 / fa_cell of that header are called from
// the kernels below as they are from the host form.
//
// The host checks the read set in one pass (fa_check: the filters, the reads' ends and their prefix maximum, the N-op refusal, the list of
// attaching I and D ops the text is printed from) and stages it.  The launches of a call, on the context's stream:
//   pileup_ops_kernel   (c3_pileup.h, shared, not copied) the per-read op table: the reference position and query offset every op starts at
//   fa_cand_kernel      one workgroup per candidate.  Two binary searches (first read with pos >= c + 17; first read whose prefix maximum of
//                       ends is > c - 16) bound the reads that can overlap; an ordered compaction (ballots, wave counts in LDS) collects the
//                       kept ones with end > c - 16 into an LDS table of kFaLdsReads entries.  Per overlapping read the centre position is
//                       resolved (fa_pos) into LDS; depth and the four base counts are fixed-order sums over the table; every attached I op
//                       is compared BASE BY BASE with every other one (the count of its string; the first of its equals stores that count
//                       for the text), D ops by length.  Over-deep: the keys of deviation (a) into LDS and a count of smaller (key, index).
//                       The row of a selected read is the count of selected reads with a smaller (haplotype, index): no sort network.
//                       Per row: the read and its allele fraction (channel 5).  No atomics anywhere
//   pileup_scan_kernel  (c3_pileup.h, shared) exclusive sums of the candidates' row counts in candidate order: rows land back to back
//   fa_fill_kernel      one workgroup per candidate, seven rows a step, one lane per (row, column): fa_pos by binary search in the read's op
//                       table, the row's insertions by column into LDS, channel 6 by looking left over at most 32 columns, one 8-byte store
//                       per cell (a row is 264 contiguous bytes).  One template on the channel count holds it and the 9-channel form of a
//                       dwell call (c3_dwell.h), whose 297-byte rows are built in LDS and written out cooperatively
// A candidate with more overlapping reads than the table holds (cfg.lds_reads lowers the cap) raises a flag: the whole call answers through
// the host form (stats: fell_back).
#pragma once
#include <hip/hip_runtime.h>
#include "c3_fa_rule.h"
#include "c3_hap_rule.h"
#include "c3_pileup.h"

namespace c3 {

#define C3_FA_TEXT __attribute__((section(".c3_fa_text")))  // behind `.c3_pileup_text`: no other kernel moves

constexpr int kFaLdsReads = 1024, kFaBlock = 256, kFaRowsAStep = 7;  // 7 x 33 = 231 lanes of 256

struct FaParams {
    FaView v;
    const int64_t *centres;
    int64_t n_cand;
    int32_t depth, cap;  // matrix_depth; overlapping reads a workgroup handles
    uint64_t seed;
    int32_t *sel_read;   // [n_cand][depth]
    int8_t *sel_af;      // [n_cand][depth]
    FaCentre *centre;    // [n_cand]
    uint32_t *ev_count;  // [n_ops], zeroed
    uint32_t *tile_n;    // [2 * n_cand]: rows, 1 for an over-deep window
    const uint32_t *tile_base;
    uint32_t *flags;     // [0]: a candidate over the cap
    int32_t *counts;     // [n_cand]
    uint64_t *rows;      // cells
};

// the number of I ops equal to op ka of read ra among the attached runs of the reads in the table; *first: none of them stands in front of it
__device__ __forceinline__ int32_t fa_count_ins(const FaView &v, const int32_t *cov, const int32_t *ins_first, const int32_t *next, int n_cov, int64_t ra,
                                                int64_t ka, bool *first) {
    int32_t n = 0;
    for (int o = 0; o < n_cov; ++o)
        for (int64_t k = ins_first[o]; k >= 0 && k < next[o]; ++k)
            if ((int)(v.cigar[k] & 15) == kOpI && fa_ins_equal(v, ra, ka, cov[o], k)) {
                ++n;
                if (cov[o] < ra || (cov[o] == ra && k < ka)) *first = false;
            }
    return n;
}

C3_FA_TEXT __global__ __launch_bounds__(kFaBlock) void fa_cand_kernel(FaParams p) {
    __shared__ int32_t cov[kFaLdsReads], c_ins_first[kFaLdsReads], c_next[kFaLdsReads], c_del_k[kFaLdsReads], c_del_len[kFaLdsReads];
    __shared__ uint64_t key[kFaLdsReads];
    __shared__ uint8_t c_state[kFaLdsReads], c_base[kFaLdsReads], c_sel[kFaLdsReads], c_hap[kFaLdsReads];
    __shared__ int32_t wave_n[kFaBlock / 64], tally[5], sel[kFaMaxDepth];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const int64_t c = p.centres[i];
    const FaView &v = p.v;
    int64_t lo, hi;
    fa_bounds(v, c, &lo, &hi);
    // the overlapping kept reads, in read order
    int n_cov = 0;
    for (int64_t base = lo; base < hi; base += kFaBlock) {  // (lo, hi and n_cov are the same in every thread)
        const int64_t r = base + tid;
        const bool mine = r < hi && fa_overlaps(v, r, c);
        const uint64_t b = __ballot(mine);
        if (lane == 0) wave_n[wave] = __popcll(b);
        __syncthreads();
        int at = n_cov, all = 0;
        for (int w = 0; w < kFaBlock / 64; ++w) at += w < wave ? wave_n[w] : 0, all += wave_n[w];
        at += __popcll(b & ((1ull << lane) - 1ull));
        if (mine && at < p.cap) cov[at] = (int32_t)r;  // (cap <= kFaLdsReads)
        n_cov += all;
        __syncthreads();
    }
    if (n_cov > p.cap) {  // the host form answers the call
        if (tid == 0) p.flags[0] = 1, p.tile_n[2 * i] = 0, p.tile_n[2 * i + 1] = 0, p.counts[i] = 0;
        return;
    }
    // the centre of every overlapping read
    for (int j = tid; j < n_cov; j += kFaBlock) {
        const FaPos f = fa_pos(v, cov[j], c);
        c_state[j] = (uint8_t)f.state, c_base[j] = (uint8_t)fa_acgt(fa_nt16_char(f.code)), c_hap[j] = v.hap[cov[j]];
        c_ins_first[j] = f.ins_first, c_next[j] = f.next, c_del_k[j] = f.del_k, c_del_len[j] = f.del_len;
    }
    __syncthreads();
    if (tid < 5) {
        int32_t n = 0;
        for (int j = 0; j < n_cov; ++j) n += tid < 4 ? (c_state[j] == 1 && c_base[j] == tid) : (c_state[j] != 0);
        tally[tid] = n;
    }
    __syncthreads();
    if (tid == 0) {
        FaCentre ce{};
        ce.depth = tally[4];
        for (int b = 0; b < 4; ++b) ce.acgt[b] = tally[b];
        p.centre[i] = ce;
    }
    // the text's records: per attached op, the number of its equals, stored by the first of them
    for (int j = tid; j < n_cov; j += kFaBlock) {
        for (int64_t k = c_ins_first[j]; k >= 0 && k < c_next[j]; ++k)
            if ((int)(v.cigar[k] & 15) == kOpI) {
                bool first = true;
                const int32_t n = fa_count_ins(v, cov, c_ins_first, c_next, n_cov, cov[j], k, &first);
                if (first) p.ev_count[k] = (uint32_t)n;
            }
        if (c_del_k[j] >= 0) {
            bool first = true;
            int32_t n = 0;
            for (int o = 0; o < n_cov; ++o)
                if (c_del_k[o] >= 0 && c_del_len[o] == c_del_len[j]) ++n, first = first && o >= j;
            if (first) p.ev_count[c_del_k[j]] = (uint32_t)n;
        }
    }
    // deviation (a): over-deep windows keep the reads of smallest (key, index)
    const bool deep = n_cov > p.depth;
    if (deep) {
        for (int j = tid; j < n_cov; j += kFaBlock) key[j] = fa_key(p.seed, c, cov[j]);
        __syncthreads();
        for (int j = tid; j < n_cov; j += kFaBlock) {
            const uint64_t k = key[j];
            int rank = 0;
            for (int o = 0; o < n_cov; ++o) rank += key[o] < k || (key[o] == k && o < j);
            c_sel[j] = rank < p.depth;
        }
    } else
        for (int j = tid; j < n_cov; j += kFaBlock) c_sel[j] = 1;
    __syncthreads();
    const int n_sel = deep ? p.depth : n_cov;
    // rows by (haplotype, index): the count of selected reads in front
    for (int j = tid; j < n_cov; j += kFaBlock)
        if (c_sel[j]) {
            int row = 0;
            for (int o = 0; o < n_cov; ++o) row += c_sel[o] && (c_hap[o] < c_hap[j] || (c_hap[o] == c_hap[j] && o < j));
            sel[row] = j;  // (row < n_sel <= depth <= kFaMaxDepth)
        }
    __syncthreads();
    const int ref_char = fa_upper(v.ref[c - v.ref_first]);
    for (int row = tid; row < n_sel; row += kFaBlock) {
        const int j = sel[row];
        const int64_t r = cov[j];
        const FaPos fc = fa_pos(v, r, c);
        int af = 0;
        bool unused = true;
        switch (fa_centre_kind(fc, ref_char)) {
        case 1: af = fa_af(fa_count_ins(v, cov, c_ins_first, c_next, n_cov, r, fc.ins_k, &unused), tally[4]); break;
        case 2: {
            int32_t n = 0;
            for (int o = 0; o < n_cov; ++o) n += c_del_k[o] >= 0 && c_del_len[o] == fc.del_len;
            af = fa_af(n, tally[4]);
            break;
        }
        case 3: af = fa_af(tally[c_base[j]], tally[4]); break;
        }
        p.sel_read[i * p.depth + row] = (int32_t)r, p.sel_af[i * p.depth + row] = (int8_t)af;
    }
    if (tid == 0) p.tile_n[2 * i] = (uint32_t)n_sel, p.tile_n[2 * i + 1] = deep ? 1u : 0u, p.counts[i] = n_sel;
}

// CH == 8: one 8-byte store per cell.  CH == 9 (cum: the dwell tables): the rows of a step, back to back in LDS, go out as bytes up to the
// first 4-byte boundary of the step's own range, whole dwords inside it and bytes behind -- the neighbouring candidate's rows start at the
// next byte, and no byte outside the step's rows is written
template <int N>
__device__ __forceinline__ uint8_t *fa_step_rows() {  // (only the 9-channel form names it: the 8-channel kernel's LDS stays as it was)
    __shared__ uint8_t s_rows[N];
    return s_rows;
}
template <int CH>
__device__ __forceinline__ void fa_fill_rows(const FaParams &p, const int32_t *cum) {
    __shared__ int32_t s_len[kFaRowsAStep][kFaPositions], s_q[kFaRowsAStep][kFaPositions];
    constexpr int kRowBytes = kFaPositions * CH;
    const int tid = threadIdx.x, slot = tid / kFaPositions, col = tid - slot * kFaPositions;
    const int64_t i = blockIdx.x;
    const int64_t c = p.centres[i], base = p.tile_base[2 * i];
    const int n = p.counts[i];
    const FaView &v = p.v;
    for (int r0 = 0; r0 < n; r0 += kFaRowsAStep) {  // (n is the same in every thread: the barriers are met by all)
        const int row = r0 + slot;
        const bool mine = slot < kFaRowsAStep && row < n;
        FaPos f;
        int64_t r = 0;
        if (mine) {
            r = p.sel_read[i * p.depth + row];
            f = fa_pos(v, r, c - kFaFlank + col);
            const bool shown = f.state == 1 && f.ins_k >= 0;
            s_len[slot][col] = shown ? f.ins_len : 0, s_q[slot][col] = shown ? f.ins_q : 0;
        }
        __syncthreads();
        if (mine) {
            const int ch6 = fa_ch6(v, r, s_len[slot], s_q[slot], col);
            if constexpr (CH == 8) p.rows[(base + row) * kFaPositions + col] = fa_cell(v, r, c - kFaFlank + col, f, p.sel_af[i * p.depth + row], ch6);
            else {
                const FaCell9 cell = fa_cell9(v, cum, r, c - kFaFlank + col, f, p.sel_af[i * p.depth + row], ch6);
                uint8_t *at = fa_step_rows<kFaRowsAStep * kRowBytes>() + slot * kRowBytes + col * CH;
                for (int b = 0; b < 8; ++b) at[b] = (uint8_t)(cell.lo >> (8 * b));
                at[8] = cell.dwell;
            }
        }
        __syncthreads();
        if constexpr (CH != 8) {
            const uint8_t *s_rows = fa_step_rows<kFaRowsAStep * kRowBytes>();
            const int n_step = n - r0 < kFaRowsAStep ? n - r0 : kFaRowsAStep, bytes = n_step * kRowBytes;
            const int64_t first = (base + r0) * kRowBytes;
            uint8_t *out = (uint8_t *)p.rows + first;  // (the buffer starts on a 4-byte boundary: hipMalloc)
            int head = (int)((4 - (first & 3)) & 3);
            head = head < bytes ? head : bytes;
            const int words = (bytes - head) >> 2, tail = head + 4 * words;
            if (tid < head) out[tid] = s_rows[tid];
            for (int w = tid; w < words; w += kFaBlock) {
                const uint8_t *b = s_rows + head + 4 * w;
                *(uint32_t *)(out + head + 4 * w) = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
            }
            if (tid < bytes - tail) out[tail + tid] = s_rows[tail + tid];
            __syncthreads();
        }
    }
}

C3_FA_TEXT __global__ __launch_bounds__(kFaBlock) void fa_fill_kernel(FaParams p) { fa_fill_rows<kFaChannels>(p, nullptr); }

}  // namespace c3

// ------------------------------------------------------------------------------------------ the context
struct c3_fa_reads_ctx {
    int device = -1;  // < 0: no GPU behind this context
    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {};
    hipEvent_t ready = nullptr, taken = nullptr;  // ready: the held device rows are complete; taken: the last ring batch has copied them
    bool taken_set = false;
    c3::FaResult host;  // the held result of the host form; after a device call its counts, depths and text (the rows stay on the device)
    bool on_host = true;
    int64_t n_cand = 0, n_rows = 0;
    c3_fa_counters stats{};
    // grown on demand, never shrunk
    c3_pileup::Buf pos, flag, mapq, cfirst, sfirst, qfirst, cigar, seq, qual, hap, kept, read_end, premax, ref, centres, op_rpos, op_q, op_read, sel_read,
        sel_af, centre, ev_count, tiles, flags, counts, rows;
    // haplotagging (c3_hap_reads.h): the tags of the last haplotag call, held on the host or (tags, alleles) on the device
    hipEvent_t hev[5] = {};
    // the dwell channel (c3_dwell.h): the staged move tables and the reads' cum tables, on the device or (host form, fallback) on the host
    hipEvent_t dev[4] = {};
    c3_pileup::Buf mv, mfirst, cum;
    std::vector<int32_t> cum_host;
    bool cum_on_host = true;
    int64_t n_cum = 0;
    c3::HapResult tagged;
    bool tags_on_host = true, hap_counted = true;
    int64_t hap_reads = 0, hap_pairs = 0, hap_ref_first = 0;  // hap_ref_first: the reference position of hap_ref's first byte
    c3_haplotag_counters hap_stats{};
    c3_pileup::Buf tags, alleles, vpos, valt, vgt, vps, pair_first, var_first, hap_ref;
    std::vector<c3_pileup::Buf *> bufs() {
        return {&pos, &flag, &mapq, &cfirst, &sfirst, &qfirst, &cigar, &seq, &qual, &hap, &kept, &read_end, &premax, &ref, &centres, &op_rpos, &op_q,
                &op_read, &sel_read, &sel_af, &centre, &ev_count, &tiles, &flags, &counts, &rows, &tags, &alleles, &vpos, &valt, &vgt, &vps,
                &pair_first, &var_first, &hap_ref, &mv, &mfirst, &cum};
    }
};

namespace c3 {

// the haplotag step of a chained call (c3_hap_reads.h): staged behind the read set, launched behind the op table; the vote kernel writes
// g->tags, which the window kernels then read as FaView::hap
struct HapJob {
    const c3_phased_variants *vars;
    const HapTables *t;
    const uint8_t *ref;
    int64_t ref_first;
};
static int hap_stage(c3_fa_reads_ctx *g, const HapJob &job, int64_t n_reads);
static int hap_launch(c3_fa_reads_ctx *g, const HapJob &job, int64_t n_reads);
static int hap_fetch_tags(c3_fa_reads_ctx *g);

// the dwell channel of a call (c3_dwell.h): the move tables are staged behind the read set, the table kernel runs beside the op table, the
// 9-channel fill kernel takes the place of fa_fill_kernel
struct DwJob {
    const c3_read_moves *moves;
    const DwTables *d;
};
static int dw_stage(c3_fa_reads_ctx *g, const DwJob &dw, int64_t n_reads);
static int dw_launch(c3_fa_reads_ctx *g, const DwJob &dw, int64_t n_reads);
static int dw_fill(c3_fa_reads_ctx *g, const FaParams &p, int64_t n_cand);

static int fa_held_on_host(c3_fa_reads_ctx *g, const c3_read_set *rs, const FaTables &t, const FaView &v, const int64_t *centres, int64_t n_cand,
                           const c3_fa_config &cfg, const DwJob *dw) {
    int64_t deep = 0;
    if (dw) fa_dwell_tables_host(rs, dw->moves, t, *dw->d, g->cum_host), g->cum_on_host = true, g->n_cum = dw->d->n_cum;
    fa_rule_host(rs, t, v, centres, n_cand, cfg, g->host, &deep, dw ? g->cum_host.data() : nullptr);
    g->on_host = true, g->stats.on_host = 1, g->stats.deep_windows = deep;
    g->stats.rows = (int64_t)(g->host.rows.size() / (size_t)(kFaPositions * g->host.channels));
    g->n_cand = n_cand, g->n_rows = g->stats.rows;
    return 0;
}

static int fa_device(c3_fa_reads_ctx *g, const c3_read_set *rs, const FaTables &t, const FaView &hv, const int64_t *centres, int64_t n_cand,
                     const c3_fa_config &cfg, const HapJob *job, const DwJob *dw) {
    HIP_TRY(hipSetDevice(g->device));
    const int64_t nr = rs->n_reads, n_ops = t.n_ops, D = cfg.matrix_depth;
    const int64_t seq_bytes = t.sfirst[(size_t)nr], qual_bytes = t.qfirst[(size_t)nr];
    const int64_t ref_lo = centres[0] - kFaFlank, ref_n = centres[n_cand - 1] + kFaFlank + 1 - ref_lo;
    hipStream_t st = g->stream;
    struct Up { c3_pileup::Buf *b; const void *src; size_t bytes; };
    const Up ups[] = {{&g->pos, rs->pos, (size_t)nr * 8}, {&g->flag, rs->flag, (size_t)nr * 2}, {&g->mapq, rs->mapq, (size_t)nr},
                      {&g->cfirst, t.cfirst.data(), (size_t)(nr + 1) * 8}, {&g->sfirst, t.sfirst.data(), (size_t)(nr + 1) * 8},
                      {&g->qfirst, t.qfirst.data(), (size_t)(nr + 1) * 8}, {&g->cigar, hv.cigar, (size_t)n_ops * 4}, {&g->seq, hv.seq, (size_t)seq_bytes},
                      {&g->qual, hv.qual, (size_t)qual_bytes}, {&g->hap, hv.hap, job ? (size_t)0 : (size_t)nr}, {&g->kept, t.kept.data(), (size_t)nr},
                      {&g->read_end, t.read_end.data(), (size_t)nr * 8}, {&g->premax, t.premax.data(), (size_t)nr * 8},
                      {&g->ref, hv.ref + (ref_lo - hv.ref_first), (size_t)ref_n}, {&g->centres, centres, (size_t)n_cand * 8}};
    for (const Up &u : ups) TRY(pileup_grow(*u.b, u.bytes));
    TRY(pileup_grow(g->op_rpos, (size_t)n_ops * 8));
    TRY(pileup_grow(g->op_q, (size_t)n_ops * 4));
    TRY(pileup_grow(g->op_read, (size_t)n_ops * 4));
    TRY(pileup_grow(g->sel_read, (size_t)(n_cand * D) * 4));
    TRY(pileup_grow(g->sel_af, (size_t)(n_cand * D)));
    TRY(pileup_grow(g->centre, (size_t)n_cand * sizeof(FaCentre)));
    TRY(pileup_grow(g->ev_count, (size_t)n_ops * 4));
    TRY(pileup_grow(g->tiles, (size_t)(4 * n_cand + 2) * 4));
    TRY(pileup_grow(g->flags, 64));
    TRY(pileup_grow(g->counts, (size_t)n_cand * 4));
    if (g->taken_set) HIP_TRY(hipStreamWaitEvent(st, g->taken, 0));  // a ring batch may still be copying the rows this call overwrites
    g->taken_set = false;
    HIP_TRY(hipEventRecord(g->ev[0], st));
    for (const Up &u : ups)
        if (u.bytes) TRY(h2d_staged(u.b->p, u.src, u.bytes, st));
    if (n_ops) HIP_TRY(hipMemsetAsync(g->ev_count.p, 0, (size_t)n_ops * 4, st));
    HIP_TRY(hipMemsetAsync(g->flags.p, 0, 64, st));
    if (job) TRY(hap_stage(g, *job, nr));
    if (dw) TRY(dw_stage(g, *dw, nr));
    HIP_TRY(hipEventRecord(g->ev[1], st));
    // the op table: pileup_ops_kernel as it is (its kept flag goes to op_read, which nothing here reads)
    PileupParams pp{};
    pp.n_reads = nr, pp.n_ops = n_ops, pp.pos = (const int64_t *)g->pos.p, pp.cigar_first = (const int64_t *)g->cfirst.p, pp.flag = (const uint16_t *)g->flag.p;
    pp.mapq = (const uint8_t *)g->mapq.p, pp.cigar = (const uint32_t *)g->cigar.p, pp.op_rpos = (int64_t *)g->op_rpos.p, pp.op_q = (int32_t *)g->op_q.p;
    pp.op_read = (int32_t *)g->op_read.p, pp.cfg.min_mq = cfg.min_mq;
    pp.tiles = n_cand, pp.tile_n = (uint32_t *)g->tiles.p, pp.tile_base = pp.tile_n + 2 * n_cand;
    if (nr > 0) PILEUP_LAUNCH(pileup_ops_kernel, (nr + 3) / 4, 256, pp);
    if (job) TRY(hap_launch(g, *job, nr));  // (its time counts under the op table here; c3_fa_haplotag_stats has it apart)
    if (dw) TRY(dw_launch(g, *dw, nr));     // (likewise; kernel_ms[7] has it apart)
    HIP_TRY(hipEventRecord(g->ev[2], st));
    FaParams p{};
    p.v.n_reads = nr, p.v.pos = pp.pos, p.v.cigar_first = pp.cigar_first, p.v.seq_first = (const int64_t *)g->sfirst.p, p.v.qual_first = (const int64_t *)g->qfirst.p;
    p.v.read_end = (const int64_t *)g->read_end.p, p.v.premax = (const int64_t *)g->premax.p, p.v.cigar = pp.cigar, p.v.flag = pp.flag, p.v.mapq = pp.mapq;
    p.v.seq = (const uint8_t *)g->seq.p, p.v.qual = (const uint8_t *)g->qual.p, p.v.hap = (const uint8_t *)(job ? g->tags.p : g->hap.p), p.v.kept = (const uint8_t *)g->kept.p;
    p.v.op_rpos = pp.op_rpos, p.v.op_q = pp.op_q, p.v.ref = (const uint8_t *)g->ref.p, p.v.ref_first = ref_lo;
    p.centres = (const int64_t *)g->centres.p, p.n_cand = n_cand, p.depth = (int32_t)D, p.seed = cfg.seed;
    p.cap = cfg.lds_reads > 0 ? std::min<int32_t>(cfg.lds_reads, kFaLdsReads) : kFaLdsReads;
    p.sel_read = (int32_t *)g->sel_read.p, p.sel_af = (int8_t *)g->sel_af.p, p.centre = (FaCentre *)g->centre.p, p.ev_count = (uint32_t *)g->ev_count.p;
    p.tile_n = pp.tile_n, p.tile_base = pp.tile_base, p.flags = (uint32_t *)g->flags.p, p.counts = (int32_t *)g->counts.p;
    PILEUP_LAUNCH(fa_cand_kernel, n_cand, kFaBlock, p);
    HIP_TRY(hipEventRecord(g->ev[3], st));
    PILEUP_LAUNCH(pileup_scan_kernel, 1, kPileupTile, pp);
    uint32_t over = 0, totals[2] = {};
    TRY(d2h_staged(&over, p.flags, 4, st));
    TRY(d2h_staged(totals, pp.tile_base + 2 * n_cand, sizeof(totals), st));
    HIP_TRY(hipEventRecord(g->ev[4], st));
    if (over) {  // a candidate with more overlapping reads than the table holds: the host form answers
        g->stats.fell_back = 1;
        if (job) TRY(hap_fetch_tags(g));  // (hv.hap is g->tagged.hap: the tags are fetched once for the host form)
        return fa_held_on_host(g, rs, t, hv, centres, n_cand, cfg, dw);
    }
    const int64_t n_rows = totals[0];
    TRY(pileup_grow(g->rows, (size_t)n_rows * (dw ? kDwRowBytes : kFaRowBytes)));
    p.rows = (uint64_t *)g->rows.p;
    if (n_rows > 0 && dw) TRY(dw_fill(g, p, n_cand));
    else if (n_rows > 0) PILEUP_LAUNCH(fa_fill_kernel, n_cand, kFaBlock, p);
    HIP_TRY(hipEventRecord(g->ev[5], st));
    HIP_TRY(hipEventRecord(g->ready, st));
    // the records the text is printed from, and the counts (the chained entry makes the slot's row table from them)
    std::vector<FaCentre> centre((size_t)n_cand);
    std::vector<uint32_t> ev_count((size_t)n_ops);
    g->host.clear();
    g->host.matrix_depth = cfg.matrix_depth, g->host.channels = dw ? kDwChannels : kFaChannels;
    g->host.count.resize((size_t)n_cand), g->host.depth.resize((size_t)n_cand);
    TRY(d2h_staged(g->host.count.data(), p.counts, (size_t)n_cand * 4, st));
    TRY(d2h_staged(centre.data(), p.centre, (size_t)n_cand * sizeof(FaCentre), st));
    if (n_ops) TRY(d2h_staged(ev_count.data(), p.ev_count, (size_t)n_ops * 4, st));
    HIP_TRY(hipEventRecord(g->ev[6], st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n_cand; ++i) g->host.depth[(size_t)i] = centre[(size_t)i].depth;
    fa_text(rs, t, centres, n_cand, centre.data(), ev_count.data(), hv.ref, hv.ref_first, cfg.max_indel_length, g->host.text);
    g->on_host = false, g->n_cand = n_cand, g->n_rows = n_rows, g->stats.rows = n_rows, g->stats.deep_windows = totals[1];
    for (int k = 0; k < 6; ++k) {  // staging in, op table, candidates, scan, fill, fetch
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, g->ev[k], g->ev[k + 1]));
        g->stats.kernel_ms[k] = ms;
    }
    for (int k = 0; dw && k < 2; ++k) {  // moves staged, dwell table
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, g->dev[2 * k], g->dev[2 * k + 1]));
        g->stats.kernel_ms[6 + k] = ms;
    }
    return 0;
}

// whatever happens next, a refusal included, the context holds no stale result
static void fa_reset(c3_fa_reads_ctx *g) {
    g->host.clear(), g->on_host = true, g->n_cand = g->n_rows = 0, g->stats = c3_fa_counters{};
    g->cum_host.clear(), g->cum_on_host = true, g->n_cum = 0;
}

static int fa_entry(c3_fa_reads_ctx *g, const c3_read_set *rs, const c3_read_extras *ex, const int64_t *centres, int64_t n_cand, const void *ref_bytes,
                    int64_t ref_first, int64_t ref_len, const c3_fa_config *cfg, bool device, const char *what, const c3_read_moves *moves = nullptr,
                    bool dwell = false) {
    if (!g) return fail("%s: null context", what);
    fa_reset(g);
    if (device && g->device < 0) return fail("%s: this context was created without a device (the _host entry needs none)", what);
    FaTables t;
    TRY(fa_check(rs, ex, centres, n_cand, ref_bytes, ref_first, ref_len, cfg, t));
    DwTables d;
    if (dwell) TRY(fa_dwell_check(moves, t, rs->n_reads, d, what));
    const DwJob dw{moves, &d};
    g->stats.reads_kept = t.n_kept, g->stats.reads_dropped = t.n_dropped, g->host.matrix_depth = cfg->matrix_depth;
    g->host.channels = dwell ? kDwChannels : kFaChannels;
    if (n_cand == 0) return 0;
    const FaView v = fa_view(rs, ex, t, (const uint8_t *)ref_bytes, ref_first);
    if (!device) return fa_held_on_host(g, rs, t, v, centres, n_cand, *cfg, dwell ? &dw : nullptr);
    return fa_device(g, rs, t, v, centres, n_cand, *cfg, nullptr, dwell ? &dw : nullptr);
}

}  // namespace c3

extern "C" {

// (the context of :496-499, :776-784: what the reference allocates per call lives here between calls)
c3_fa_reads_ctx *c3_fa_reads_create(int device) {
    using namespace c3;
    c3_fa_reads_ctx *g = new c3_fa_reads_ctx();
    if (device < 0) return g;
    const int ndev = c3_device_count();
    bool ok = false;
    if (ndev <= 0) fail("c3_fa_reads_create: no HIP device visible (a context with device < 0 and c3_fa_reads_host need none)");
    else if (device >= ndev) fail("c3_fa_reads_create: device %d out of range (%d visible)", device, ndev);
    else if (hipSetDevice(device) != hipSuccess) fail("hipSetDevice(%d) failed", device);
    else if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) fail("c3_fa_reads_create: hipStreamCreate failed");
    else {
        ok = true;
        for (hipEvent_t &e : g->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        for (hipEvent_t &e : g->hev) ok = ok && hipEventCreate(&e) == hipSuccess;
        for (hipEvent_t &e : g->dev) ok = ok && hipEventCreate(&e) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&g->ready, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&g->taken, hipEventDisableTiming) == hipSuccess;
        if (!ok) fail("c3_fa_reads_create: hipEventCreate failed");
    }
    if (!ok) {
        for (hipEvent_t e : g->ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : g->hev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : g->dev)
            if (e) (void)hipEventDestroy(e);
        if (g->ready) (void)hipEventDestroy(g->ready);
        if (g->taken) (void)hipEventDestroy(g->taken);
        if (g->stream) (void)hipStreamDestroy(g->stream);
        delete g;
        return nullptr;
    }
    g->device = device;
    return g;
}

int c3_fa_reads_destroy(c3_fa_reads_ctx *g) {
    if (!g) return 0;
    if (g->device >= 0) {
        (void)hipSetDevice(g->device);
        if (g->stream) (void)hipStreamSynchronize(g->stream), (void)hipStreamDestroy(g->stream);
        for (hipEvent_t e : g->ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : g->hev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : g->dev)
            if (e) (void)hipEventDestroy(e);
        if (g->ready) (void)hipEventDestroy(g->ready);
        if (g->taken) (void)hipEventDestroy(g->taken);
        for (c3_pileup::Buf *b : g->bufs())
            if (b->p) (void)hipFree(b->p);
    }
    delete g;
    return 0;
}

// the device form of the candidate loop :787-1008 (and of the read loop :535-774 behind the filters, which the host applies)
int c3_fa_reads(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const int64_t *centres, int64_t n_cand, const void *ref_bytes,
                int64_t ref_first, int64_t ref_len, const c3_fa_config *cfg) {
    return c3::fa_entry(g, reads, extras, centres, n_cand, ref_bytes, ref_first, ref_len, cfg, true, "c3_fa_reads");
}

// :535-1008 as sequential host C
int c3_fa_reads_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const int64_t *centres, int64_t n_cand,
                     const void *ref_bytes, int64_t ref_first, int64_t ref_len, const c3_fa_config *cfg) {
    return c3::fa_entry(g, reads, extras, centres, n_cand, ref_bytes, ref_first, ref_len, cfg, false, "c3_fa_reads_host");
}

int c3_fa_reads_sizes(c3_fa_reads_ctx *g, int64_t *n_cand, int64_t *n_rows, int64_t *text_bytes, int32_t *matrix_depth) {
    if (!g) return fail("c3_fa_reads_sizes: null context");
    if (n_cand) *n_cand = g->n_cand;
    if (n_rows) *n_rows = g->n_rows;
    if (text_bytes) *text_bytes = (int64_t)g->host.text.size();
    if (matrix_depth) *matrix_depth = g->host.matrix_depth;
    return 0;
}

// data->matrix (as rows) and data->all_alt_info of :1011-1013
int c3_fa_reads_result(c3_fa_reads_ctx *g, void *rows, int32_t *counts, int32_t *depths, char *text) {
    using namespace c3;
    if (!g) return fail("c3_fa_reads_result: null context");
    const FaResult &h = g->host;
    if (text && !h.text.empty()) memcpy(text, h.text.data(), h.text.size());
    if (counts && !h.count.empty()) memcpy(counts, h.count.data(), h.count.size() * 4);
    if (depths && !h.depth.empty()) memcpy(depths, h.depth.data(), h.depth.size() * 4);
    if (!rows || g->n_rows == 0) return 0;
    if (g->on_host) return memcpy(rows, h.rows.data(), h.rows.size()), 0;
    HIP_TRY(hipSetDevice(g->device));
    return d2h_staged(rows, g->rows.p, (size_t)g->n_rows * kFaPositions * h.channels, g->stream);
}

int c3_fa_reads_stats(c3_fa_reads_ctx *g, c3_fa_counters *out) {
    if (!g || !out) return fail("c3_fa_reads_stats: null argument");
    *out = g->stats;
    return 0;
}

int c3_fa_lds_reads(void) { return c3::kFaLdsReads; }

// ---- the chained entry: the held rows as a rows batch of the ring (c3_hostring.h).  The rows go from the context's buffer to the slot by one
// device-to-device copy on the lane's stream; the slot's row table is made on the host from the counts, which came back with the call.  From
// there on the batch is a batch of c3_predict_submit_rows (row_first == NULL).  A held result of the host form goes through that entry itself
int c3_predict_submit_fa_reads(c3_model *m, c3_fa_reads_ctx *g, float *y_host, int64_t *n_rows_host, int slot) {
    using namespace c3;
    TRY(ring_ready(m, slot));
    if (!g) return fail("c3_predict_submit_fa_reads: null context");
    if (m->kind != C3_KIND_FULL_ALIGNMENT) return fail("c3_predict_submit_fa_reads: full-alignment windows need a full-alignment model, this is a pileup handle");
    if (m->C != g->host.channels)
        return fail("c3_predict_submit_fa_reads: the handle has %d channels; the held windows have %d (c3_fa_reads builds 8, c3_fa_reads_dwell 9 with the dwell channel)",
                    m->C, g->host.channels);
    if (m->positions != kFaPositions) return fail("c3_predict_submit_fa_reads: the handle has %d positions, the windows %d", m->positions, kFaPositions);
    if (m->depth != g->host.matrix_depth)
        return fail("c3_predict_submit_fa_reads: the handle's depth is %d rows, the held result was built for matrix_depth %d", m->depth, g->host.matrix_depth);
    const int64_t batch = g->n_cand;
    if (n_rows_host) *n_rows_host = batch;
    if (g->on_host || g->n_rows == 0)
        return c3_predict_submit_rows(m, g->host.rows.empty() ? (const void *)g->host.count.data() : (const void *)g->host.rows.data(), nullptr,
                                      g->host.count.data(), batch, y_host, slot);
    if (g->device != m->device) return fail("c3_predict_submit_fa_reads: the context is on device %d, the model on device %d", g->device, m->device);
    if (!y_host) return fail("null buffer: y_host");
    RingInput in = ring_input(InKind::Rows, g->rows.p, C3_DTYPE_I8, batch, y_host);
    in.row_count = g->host.count.data(), in.rows_total = g->n_rows;
    in.dev_rows = g->rows.p, in.dev_ready = g->ready, in.dev_taken = g->taken;
    g->taken_set = true;  // (queue_device_rows records it behind its copy; set first: a submit that fails behind it leaves the event recorded)
    return predict_submit(m, in, slot);
}

int c3_predict_fa_reads(c3_model *m, c3_fa_reads_ctx *g, float *y_host, int64_t *n_rows_host) {
    TRY(c3_predict_submit_fa_reads(m, g, y_host, n_rows_host, 0));
    return c3_predict_wait(m, 0);
}

}  // extern "C"
