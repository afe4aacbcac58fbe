// c3_dwell.h -- the dwell channel on the device: the 9-channel windows of enable_dwell_time (src/clair3_full_alignment_dwell.c) from a
// c3_read_set, its c3_read_extras and the reads' move tables (c3_read_moves).  The rule and the host form: c3_dwell_rule.h; fa_dwell_value /
// fa_cell9 of that header are called from the fill kernel as they are from the host form.
//
// The move tables (2 - 3 bytes a base: the largest array a call stages) and their offsets are staged behind the read set on the context's
// stream.  The launches a dwell call adds or replaces:
//   fa_dwell_kernel     one workgroup of 256 lanes per read: the read's table into its prefix array cum[0 .. l] (c3_dwell_rule.h).  It walks
//                       the table in steps of kDwStep bytes, 16 bytes a lane; a step starts at the 16-byte boundary at or in front of the
//                       table's first byte (reads are packed back to back, so a table starts at any byte address), so that every lane's
//                       16 bytes are one aligned load where they lie inside the table and single bytes at its head and tail.  A lane
//                       counts its non-zero bytes; the ranks come from an ordered scan (lane shuffles inside a wave, wave totals in LDS)
//                       and a carry from step to step; a non-zero entry of rank k <= l stores its index at cum[k], the entry of rank 0 also
//                       as n_0.  The walk ends with the table or once more than l entries are ranked (the reference's `break`).  Then,
//                       in the same launch, every lane takes the pairs (q, l - q): cum[q] = n_q - n_0 below K, L - n_0 from K on, and for a
//                       read with flag & 16 cum_rev[q] = cum[l] - cum[l - q].  No atomics, no scratch
//   fa_fill9_kernel     fa_fill_rows<9> (c3_fa_reads.h) in the place of fa_fill_kernel: rows of 297 bytes
// A tiled two-pass form over the concatenated tables (pileup_scan_kernel) would balance ultra-long reads better; it is not built
// (profiles/fa_dwell.txt has what the one-workgroup-per-read kernel costs).
#pragma once
#include <hip/hip_runtime.h>
#include "c3_dwell_rule.h"
#include "c3_hap_reads.h"

namespace c3 {

#define C3_DWELL_TEXT __attribute__((section(".c3_dwell_text")))  // behind `.c3_hap_text`: no other kernel moves

constexpr int kDwBlock = 256, kDwLaneBytes = 16, kDwStep = kDwBlock * kDwLaneBytes;  // 4096

struct DwParams {
    const int64_t *mfirst, *qfirst;  // [n + 1] each, rebased
    const uint16_t *flag;
    const int8_t *mv;
    int32_t *cum;  // read r at cum + qfirst[r] + r, l + 1 entries
};

C3_DWELL_TEXT __global__ __launch_bounds__(kDwBlock) void fa_dwell_kernel(DwParams p) {
    __shared__ int32_t wave_n[kDwBlock / 64], s_n0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int64_t A = p.mfirst[r], L = p.mfirst[r + 1] - A, q0 = p.qfirst[r], l = p.qfirst[r + 1] - q0;
    int32_t *cum = p.cum + q0 + r;
    if (L <= 1 || l == 0) {  // no table (the same in every lane)
        for (int64_t q = tid; q <= l; q += kDwBlock) cum[q] = 0;
        return;
    }
    const bool reverse = (p.flag[r] & 16) != 0;
    const int64_t lo = A + 1, hi = A + L;  // the entries that count, as bytes of the staged array: element 0 is skipped
    int64_t K = 0;                         // non-zero entries in front of this step (the same in every lane)
    for (int64_t w0 = A & ~(int64_t)(kDwLaneBytes - 1); w0 < hi && K <= l; w0 += kDwStep) {
        const int64_t w = w0 + (int64_t)kDwLaneBytes * tid;
        uint32_t m = 0;  // bit b: byte w + b counts and is non-zero
        if (w >= lo && w + kDwLaneBytes <= hi) {
            const uint4 x = *(const uint4 *)(p.mv + w);  // (w is a multiple of 16 and the staged array starts on one)
            const uint32_t d[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < 4; ++b) m |= ((d[j] >> (8 * b)) & 255u ? 1u : 0u) << (4 * j + b);
        } else {
            for (int b = 0; b < kDwLaneBytes; ++b)
                if (w + b >= lo && w + b < hi && p.mv[w + b] != 0) m |= 1u << b;
        }
        const int mine = __popc(m);
        int upto = mine;  // the inclusive sum over the lanes of the wave
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(upto, off, 64);
            if (lane >= off) upto += o;
        }
        if (lane == 63) wave_n[wave] = upto;
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < kDwBlock / 64; ++k) before += k < wave ? wave_n[k] : 0, all += wave_n[k];
        int64_t rank = K + before + upto - mine;
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            if (rank == 0) s_n0 = (int32_t)(w + b - A);
            if (rank <= l) cum[rank] = (int32_t)(w + b - A);  // (ranks above l are the bases the reference drops)
            ++rank;
        }
        K += all;
        __syncthreads();  // (wave_n is written again in the next step; behind the last step: the indices are visible to every lane)
    }
    const int32_t n0 = K > 0 ? s_n0 : 0, end = K > 0 ? (int32_t)L - n0 : 0;
    const int32_t total = l < K ? cum[l] - n0 : end;
    __syncthreads();  // every lane has read cum[l] before the pass below overwrites it
    for (int64_t q = tid; 2 * q <= l; q += kDwBlock) {  // the pair (q, l - q) is read and written by this lane alone
        const int64_t o = l - q;
        const int32_t a = q < K ? cum[q] - n0 : end, b = o < K ? cum[o] - n0 : end;
        if (reverse) cum[q] = total - b, cum[o] = total - a;
        else cum[q] = a, cum[o] = b;
    }
}

C3_DWELL_TEXT __global__ __launch_bounds__(kFaBlock) void fa_fill9_kernel(FaParams p, const int32_t *cum) { fa_fill_rows<kDwChannels>(p, cum); }

// ------------------------------------------------------------------------------------------ staging and launches
static int dw_stage(c3_fa_reads_ctx *g, const DwJob &dw, int64_t n_reads) {
    const DwTables &d = *dw.d;
    hipStream_t st = g->stream;
    TRY(pileup_grow(g->mv, (size_t)d.n_moves));
    TRY(pileup_grow(g->mfirst, (size_t)(n_reads + 1) * 8));
    TRY(pileup_grow(g->cum, (size_t)d.n_cum * 4));
    HIP_TRY(hipEventRecord(g->dev[0], st));
    TRY(h2d_staged(g->mfirst.p, d.mfirst.data(), (size_t)(n_reads + 1) * 8, st));
    if (d.n_moves) TRY(h2d_staged(g->mv.p, dw.moves->mv + d.m_base, (size_t)d.n_moves, st));
    HIP_TRY(hipEventRecord(g->dev[1], st));
    return 0;
}

// behind the staged read set (g->qfirst and g->flag hold this call's reads)
static int dw_launch(c3_fa_reads_ctx *g, const DwJob &dw, int64_t n_reads) {
    hipStream_t st = g->stream;
    DwParams p{};
    p.mfirst = (const int64_t *)g->mfirst.p, p.qfirst = (const int64_t *)g->qfirst.p, p.flag = (const uint16_t *)g->flag.p;
    p.mv = (const int8_t *)g->mv.p, p.cum = (int32_t *)g->cum.p;
    HIP_TRY(hipEventRecord(g->dev[2], st));
    if (n_reads > 0) PILEUP_LAUNCH(fa_dwell_kernel, n_reads, kDwBlock, p);
    HIP_TRY(hipEventRecord(g->dev[3], st));
    g->cum_on_host = false, g->n_cum = dw.d->n_cum;
    return 0;
}

static int dw_fill(c3_fa_reads_ctx *g, const FaParams &p, int64_t n_cand) {
    PILEUP_LAUNCH(fa_fill9_kernel, n_cand, kFaBlock, p, (const int32_t *)g->cum.p);
    return 0;
}

static int dw_entry(c3_fa_reads_ctx *g, const c3_read_set *rs, const c3_read_extras *ex, const c3_read_moves *moves, const c3_phased_variants *vs,
                    const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first, int64_t ref_len, const c3_fa_config *cfg,
                    const c3_haplotag_config *hcfg, bool device, const char *what) {
    if (!g) return fail("%s: null context", what);
    if ((vs != nullptr) != (hcfg != nullptr)) {
        fa_reset(g), hap_reset(g);
        return fail("%s: variants and hap_cfg are both NULL or both given", what);
    }
    if (!moves) {
        fa_reset(g);
        return fail("%s: null moves", what);
    }
    if (vs) return fa_phased_entry(g, rs, ex, vs, centres, n_cand, ref_bytes, ref_first, ref_len, cfg, hcfg, device, what, moves, true);
    return fa_entry(g, rs, ex, centres, n_cand, ref_bytes, ref_first, ref_len, cfg, device, what, moves, true);
}

}  // namespace c3

extern "C" {

int c3_fa_reads_dwell(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_read_moves *moves,
                      const c3_phased_variants *variants, const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first,
                      int64_t ref_len, const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg) {
    return c3::dw_entry(g, reads, extras, moves, variants, centres, n_cand, ref_bytes, ref_first, ref_len, fa_cfg, hap_cfg, true, "c3_fa_reads_dwell");
}

int c3_fa_reads_dwell_host(c3_fa_reads_ctx *g, const c3_read_set *reads, const c3_read_extras *extras, const c3_read_moves *moves,
                           const c3_phased_variants *variants, const int64_t *centres, int64_t n_cand, const void *ref_bytes, int64_t ref_first,
                           int64_t ref_len, const c3_fa_config *fa_cfg, const c3_haplotag_config *hap_cfg) {
    return c3::dw_entry(g, reads, extras, moves, variants, centres, n_cand, ref_bytes, ref_first, ref_len, fa_cfg, hap_cfg, false,
                        "c3_fa_reads_dwell_host");
}

int c3_fa_reads_channels(c3_fa_reads_ctx *g) { return g ? g->host.channels : c3::kFaChannels; }

int c3_fa_dwell_cum_host(const int8_t *mv, int64_t L, int64_t l, int reverse, int32_t *cum_out) {
    if (l < 0 || L < 0 || !cum_out || (L > 0 && !mv)) return fail("c3_fa_dwell_cum_host: a negative length or a null array"), 0;
    return c3::fa_dwell_cum_host(mv, L, l, reverse != 0, cum_out) ? 1 : 0;
}

int64_t c3_fa_dwell_table(c3_fa_reads_ctx *g, int32_t *cum_out) {
    using namespace c3;
    if (!g) return fail("c3_fa_dwell_table: null context"), -1;
    if (!cum_out || g->n_cum == 0) return g->n_cum;
    if (g->cum_on_host) return memcpy(cum_out, g->cum_host.data(), (size_t)g->n_cum * 4), g->n_cum;
    if (hipSetDevice(g->device) != hipSuccess) return fail("hipSetDevice(%d) failed", g->device), -1;
    if (d2h_staged(cum_out, g->cum.p, (size_t)g->n_cum * 4, g->stream)) return -1;
    return g->n_cum;
}

int c3_fa_dwell_step(void) { return c3::kDwStep; }

}  // extern "C"
