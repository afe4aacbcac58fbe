// c3_pileup.h -- pileup from reads on the device: the region matrix, major, the candidates with their alt-info and the gVCF count pair of
// calculate_clair3_pileup (src/clair3_pileup.c:208-461) from a c3_read_set.  The rule and the host form: c3_pileup_rule.h; the per-column
// arithmetic is that header's pileup_site(), called from the kernels below as it is from the host form.
//
// The launches of a call, on the context's stream.  Every sum is an integer sum and every maximum an integer maximum, so the images do not
// depend on the order in which the adds arrive:
//   pileup_ops_kernel      one wave per read scans its CIGAR 64 ops a step: per op the exclusive prefix of reference and query consumption
//                          (as the absolute reference position and the query offset the op starts at) and its read, -1 for a dropped read
//   pileup_walk_kernel     one lane per op loops over the op's bases clipped to the region and adds into the dense (end - start) x 18 int32
//                          image: the base channels, 8 / 17 for deleted bases.  Bases that count in no channel add into a side image (depth
//                          is the row's sum plus that), N ops store into the span image.  The shape of these adds is the UNCOALESCED one of
//                          the HIP guide's Guideline 12: every lane issues one 4-byte atomic into a 72-byte row of its own, and the rows of
//                          consecutive ops lie as far apart as the ops are long (tens of rows at a sequencing error rate of a per cent or
//                          two); a lane also loops over its whole op, so an op of 5 000 matching bases is 5 000 serial steps of one lane.
//                          A form that privatises a tile of positions in LDS, or gives a long op to a wave, was not built: the walk is
//                          1.4 - 6 ms of calls of 37 - 200 ms (profiles/pileup_reads.txt)
//                          An I or D op that is an event of the rule (its nearest op in front, P skipped, is M, =, X or D, and ends inside
//                          the region) is counted in the event table: open addressing in global memory, a 64-bit key mixed from column,
//                          strand, kind, length and a hash of the inserted bases, ANDed with hash_mask, claimed with a 64-bit compare-and-swap;
//                          the count is a 32-bit atomic add; the claiming lane stores its op as the slot's representative.  The table holds
//                          at least twice the I and D ops of the kept reads (counted by the host while it checks the read set): it cannot
//                          fill.  Deletion starts live in the same table: their key carries no base hash
//   pileup_verify_kernel   a launch of its own, so that no representative is read while it is written: every event compares its column,
//                          strand, kind, length and bases with its slot's representative; a difference sets the collision flag.  Results
//                          never rest on the keys being unique: a call whose flag is set answers through the host form (stats: fell_back)
//   pileup_reduce_kernel   one lane per slot: adds into channels 4 / 6 / 13 / 15, takes the maximum into 5 / 7 / 14 / 16
//   pileup_exist_kernel    per site: raw depth, whether a column exists
//   pileup_site_kernel     per site: pileup_site(), the flanking test from the 16 existence flags to its left, the count pair
//   pileup_count_kernel / pileup_scan_kernel / pileup_emit_kernel   order-preserving compaction (the pattern of c3_gvcf.h): existing columns
//                          to the region matrix (reference base's channels negated here) and major, candidates to fixed-size records
//   pileup_alleles_kernel  slots at candidate columns to allele records; these are appended through one atomic counter, in no fixed order:
//                          the host sorts and merges them anyway (they are few), decodes the representatives' bases and prints the lines
#pragma once
#include <hip/hip_runtime.h>
#include "c3_pileup_rule.h"

namespace c3 {

#define C3_PILEUP_TEXT __attribute__((section(".c3_pileup_text")))  // behind `.c3_gvcf_text`: no other kernel moves

constexpr int kPileupTile = 1024;
constexpr uint64_t kPileupEmpty = ~0ull;

struct PileupCandRec {  // 40 bytes
    int64_t pos;
    int32_t depth, ref_depth;
    int32_t x[4];
    uint8_t ref_base, r, pad[6];
};
struct PileupAlleleRec {  // 24 bytes
    int32_t cand, len, read, q;
    uint32_t count;
    uint8_t ins, rev, pad[2];
};

struct PileupParams {
    c3_pileup_config cfg;
    int64_t start, end, n;  // n = end - start
    int64_t n_reads, n_ops;
    // the read set
    const int64_t *pos, *cigar_first, *seq_first;  // cigar_first is rebased: [0] = 0
    const uint16_t *flag;
    const uint8_t *mapq, *seq;
    const uint32_t *cigar;
    const uint8_t *ref;  // the reference bytes of [start, end)
    // per op
    int64_t *op_rpos;
    int32_t *op_q, *op_read, *ev_slot;
    // the event table
    uint64_t *key;
    uint32_t *cnt, *rep;
    uint32_t cap;  // a power of two
    // per site
    int32_t *img, *other, *depth, *cand_index;
    uint8_t *span, *flags;  // flags: 1 a column exists, 2 a candidate
    int64_t *n_ref, *n_total;
    uint32_t *tile_n, *tile_base;  // [2 * tiles] / [2 * tiles + 2]: columns, candidates
    int64_t tiles;
    uint32_t *scalars;  // [0] collision flag [1] collisions [2] events [3] allele records [4] a probe that found no slot
    // compacted
    int32_t *out_matrix, *out_cdepth;
    int64_t *out_major, *out_cpos;
    PileupCandRec *out_cand;
    PileupAlleleRec *out_allele;
    int64_t allele_cap;
};

__device__ __forceinline__ uint64_t pileup_mix(uint64_t x) {  // the finaliser of splitmix64
    x ^= x >> 30, x *= 0xbf58476d1ce4e5b9ull, x ^= x >> 27, x *= 0x94d049bb133111ebull, x ^= x >> 31;
    return x;
}

C3_PILEUP_TEXT __global__ __launch_bounds__(256) void pileup_ops_kernel(PileupParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.n_reads) return;  // (wave-uniform)
    const bool kept = pileup_kept(p.flag[r], p.mapq[r], p.cfg.min_mq);
    const int64_t c0 = p.cigar_first[r], c1 = p.cigar_first[r + 1];
    int32_t ref_carry = 0, q_carry = 0;
    const int64_t pos = p.pos[r];
    for (int64_t base = c0; base < c1; base += 64) {
        const int64_t k = base + lane;
        int32_t rl = 0, ql = 0;
        if (k < c1) {
            const uint32_t c = p.cigar[k];
            const int op = (int)(c & 15);
            if (pileup_op_ref(op)) rl = (int32_t)(c >> 4);
            if (pileup_op_query(op)) ql = (int32_t)(c >> 4);
        }
        int32_t rs = rl, qs = ql;
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t a = __shfl_up(rs, off, 64), b = __shfl_up(qs, off, 64);
            if (lane >= off) rs += a, qs += b;
        }
        if (k < c1) {
            p.op_rpos[k] = pos + ref_carry + (rs - rl);
            p.op_q[k] = q_carry + (qs - ql);
            p.op_read[k] = kept ? (int32_t)r : -1;
        }
        ref_carry += __shfl(rs, 63, 64), q_carry += __shfl(qs, 63, 64);
    }
}

// the event an I or D op k of a kept read stands for, if any: column, length (the consecutive I ops behind an I added up)
__device__ __forceinline__ bool pileup_event(const PileupParams &p, int64_t k, int32_t read, int64_t *col, int32_t *len) {
    const uint32_t c = p.cigar[k];
    const int op = (int)(c & 15);
    const int64_t c0 = p.cigar_first[read], c1 = p.cigar_first[read + 1];
    int64_t j = k - 1;
    while (j >= c0 && (int)(p.cigar[j] & 15) == kOpP) --j;
    if (j < c0 || !pileup_op_anchor((int)(p.cigar[j] & 15))) return false;
    const int64_t at = p.op_rpos[k] - 1;  // the anchor's last reference position (P consumes nothing)
    if (at < p.start || at >= p.end) return false;
    int32_t total = (int32_t)(c >> 4);
    if (op == kOpI)
        for (int64_t i = k + 1; i < c1 && (int)(p.cigar[i] & 15) == kOpI; ++i) total += (int32_t)(p.cigar[i] >> 4);
    *col = at - p.start, *len = total;
    return true;
}

C3_PILEUP_TEXT __global__ __launch_bounds__(256) void pileup_walk_kernel(PileupParams p) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= p.n_ops) return;
    const int32_t read = p.op_read[k];
    int32_t slot_of = -1;
    if (read >= 0) {
        const uint32_t c = p.cigar[k];
        const int op = (int)(c & 15);
        const int64_t len = c >> 4, rp = p.op_rpos[k];
        const int rev = (p.flag[read] & 16) ? 9 : 0;
        const int64_t lo = max(rp, p.start), hi = min(rp + len, p.end);  // (lo >= start, hi <= end: every row below is inside the image)
        if (pileup_op_base(op)) {
            const int64_t sf = p.seq_first[read], q0 = (int64_t)p.op_q[k] - rp;
            for (int64_t at = lo; at < hi; ++at) {
                const int ch = pileup_channel(pileup_code(p.seq, sf, q0 + at));
                if (ch >= 0) atomicAdd(&p.img[(at - p.start) * kPileupChannels + ch + rev], 1);
                else atomicAdd(&p.other[at - p.start], 1);
            }
        } else if (op == kOpD) {
            for (int64_t at = lo; at < hi; ++at) atomicAdd(&p.img[(at - p.start) * kPileupChannels + 8 + rev], 1);
        } else if (op == kOpN) {
            for (int64_t at = lo; at < hi; ++at) p.span[at - p.start] = 1;  // (every writer stores the same 1)
        }
        int64_t col;
        int32_t total;
        if ((op == kOpI || op == kOpD) && pileup_event(p, k, read, &col, &total)) {
            uint64_t h = 0;
            if (op == kOpI) {
                const int64_t sf = p.seq_first[read], q = p.op_q[k];
                for (int32_t i = 0; i < total; ++i) h = (h ^ (uint64_t)pileup_code(p.seq, sf, q + i)) * 0x100000001b3ull + 0x9e3779b97f4a7c15ull;
            }
            const uint64_t id = (uint64_t)col | (uint64_t)(rev ? 1 : 0) << 40 | (uint64_t)(op == kOpI ? 1 : 0) << 41;
            const uint64_t key = (pileup_mix(id) ^ pileup_mix(h + (uint64_t)(uint32_t)total * 0xd6e8feb86659fd93ull)) & p.cfg.hash_mask & ~(1ull << 63);  // (never kPileupEmpty)
            uint32_t s = (uint32_t)pileup_mix(key ^ 0x2545f4914f6cdd1dull) & (p.cap - 1);
            uint32_t tries = 0;
            for (; tries < p.cap; ++tries, s = (s + 1) & (p.cap - 1)) {
                const uint64_t seen = atomicCAS((unsigned long long *)&p.key[s], (unsigned long long)kPileupEmpty, (unsigned long long)key);
                if (seen == kPileupEmpty) p.rep[s] = (uint32_t)k;
                if (seen == kPileupEmpty || seen == key) {
                    atomicAdd(&p.cnt[s], 1u);
                    slot_of = (int32_t)s;
                    break;
                }
            }
            if (tries == p.cap) atomicAdd(&p.scalars[4], 1u);
            atomicAdd(&p.scalars[2], 1u);
        }
    }
    p.ev_slot[k] = slot_of;
}

C3_PILEUP_TEXT __global__ __launch_bounds__(256) void pileup_verify_kernel(PileupParams p) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= p.n_ops) return;
    const int32_t s = p.ev_slot[k];
    if (s < 0) return;
    const int64_t j = p.rep[s];
    if (j == k) return;
    const int32_t ra = p.op_read[k], rb = p.op_read[j];
    int64_t col_a = 0, col_b = 0;
    int32_t len_a = 0, len_b = 0;
    bool same = rb >= 0 && pileup_event(p, k, ra, &col_a, &len_a) && pileup_event(p, j, rb, &col_b, &len_b);
    same = same && col_a == col_b && len_a == len_b && (p.cigar[k] & 15) == (p.cigar[j] & 15) && ((p.flag[ra] ^ p.flag[rb]) & 16) == 0;
    if (same && (int)(p.cigar[k] & 15) == kOpI) {
        const int64_t sa = p.seq_first[ra], sb = p.seq_first[rb], qa = p.op_q[k], qb = p.op_q[j];
        for (int32_t i = 0; i < len_a && same; ++i) same = pileup_code(p.seq, sa, qa + i) == pileup_code(p.seq, sb, qb + i);
    }
    if (!same) atomicOr(&p.scalars[0], 1u), atomicAdd(&p.scalars[1], 1u);
}

C3_PILEUP_TEXT __global__ __launch_bounds__(256) void pileup_reduce_kernel(PileupParams p) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= p.cap || p.key[s] == kPileupEmpty) return;
    const int64_t k = p.rep[s];
    const int32_t read = p.op_read[k];
    const int64_t col = p.op_rpos[k] - 1 - p.start;
    if (read < 0 || col < 0 || col >= p.n) return;  // (an event's column is inside the region by construction)
    const int ch = ((int)(p.cigar[k] & 15) == kOpI ? 4 : 6) + ((p.flag[read] & 16) ? 9 : 0);
    const int32_t c = (int32_t)p.cnt[s];
    atomicAdd(&p.img[col * kPileupChannels + ch], c);
    atomicMax(&p.img[col * kPileupChannels + ch + 1], c);
}

C3_PILEUP_TEXT __global__ __launch_bounds__(256) void pileup_exist_kernel(PileupParams p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int32_t d = pileup_raw_depth(p.img + i * kPileupChannels, p.other[i]);
    p.depth[i] = d;
    p.flags[i] = (d > 0 || p.span[i]) ? 1 : 0;
}

C3_PILEUP_TEXT __global__ __launch_bounds__(256) void pileup_site_kernel(PileupParams p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    int64_t nr = 0, nt = 0;
    if (p.flags[i] & 1) {
        int32_t m[kPileupChannels];
        for (int c = 0; c < kPileupChannels; ++c) m[c] = p.img[i * kPileupChannels + c];
        const PileupSite s = pileup_site(m, p.depth[i], p.ref[i], p.cfg);
        // contiguous_flanking_num >= 16: sixteen columns directly to the left, none of them position 0 (:225-229)
        bool flank = i >= kPileupFlank && p.start + i - kPileupFlank != 0;
        for (int j = 1; j <= kPileupFlank && flank; ++j) flank = (p.flags[i - j] & 1) != 0;
        if (s.pass && (p.cfg.call_ht || flank)) p.flags[i] = 3;  // (bit 0 is all a neighbour reads, and it does not change)
        nr = s.ref_count, nt = (int64_t)s.ref_count + s.all_alt + s.del_count + s.ins_count;
    }
    if (p.cfg.gvcf) p.n_ref[i] = nr, p.n_total[i] = nt;
}

C3_PILEUP_TEXT __global__ __launch_bounds__(kPileupTile) void pileup_count_kernel(PileupParams p) {
    __shared__ uint32_t wave_n[2][kPileupTile / 64];
    const int64_t i = (int64_t)blockIdx.x * kPileupTile + threadIdx.x;
    const uint8_t f = i < p.n ? p.flags[i] : 0;
    const uint64_t a = __ballot(f & 1), b = __ballot(f & 2);
    if ((threadIdx.x & 63) == 0) wave_n[0][threadIdx.x >> 6] = (uint32_t)__popcll(a), wave_n[1][threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t s = 0;
        for (int w = 0; w < kPileupTile / 64; ++w) s += wave_n[threadIdx.x][w];
        p.tile_n[2 * blockIdx.x + threadIdx.x] = s;
    }
}

// exclusive sums of the tiles' two counts in tile order, one workgroup, 1024 tiles a step; tile_base[2 * tiles + which] = all
C3_PILEUP_TEXT __global__ __launch_bounds__(kPileupTile) void pileup_scan_kernel(PileupParams p) {
    __shared__ uint32_t a[kPileupTile];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x;
    for (int which = 0; which < 2; ++which) {
        if (tid == 0) carry = 0;
        __syncthreads();
        for (int64_t c0 = 0; c0 < p.tiles; c0 += kPileupTile) {
            const int64_t t = c0 + tid;
            const uint32_t own = t < p.tiles ? p.tile_n[2 * t + which] : 0u;
            a[tid] = own;
            __syncthreads();
            for (int off = 1; off < kPileupTile; off <<= 1) {
                const uint32_t v = tid >= off ? a[tid - off] : 0u;
                __syncthreads();
                a[tid] += v;
                __syncthreads();
            }
            const uint32_t base = carry;
            if (t < p.tiles) p.tile_base[2 * t + which] = base + a[tid] - own;
            __syncthreads();
            if (tid == kPileupTile - 1) carry = base + a[tid];
            __syncthreads();
        }
        if (tid == 0) p.tile_base[2 * p.tiles + which] = carry;
        __syncthreads();
    }
}

// column of site i goes to slot (columns in front of its tile) + (in front of its wave) + (in front of its lane); candidates alike
C3_PILEUP_TEXT __global__ __launch_bounds__(kPileupTile) void pileup_emit_kernel(PileupParams p) {
    __shared__ uint32_t wave_n[2][kPileupTile / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * kPileupTile + tid;
    const uint8_t f = i < p.n ? p.flags[i] : 0;
    const uint64_t a = __ballot(f & 1), b = __ballot(f & 2);
    if (lane == 0) wave_n[0][wave] = (uint32_t)__popcll(a), wave_n[1][wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (i >= p.n) return;
    int32_t ci = -1;
    if (f & 1) {
        int64_t slot = p.tile_base[2 * blockIdx.x];
        for (int w = 0; w < wave; ++w) slot += wave_n[0][w];
        slot += __popcll(a & ((1ull << lane) - 1ull));
        int32_t m[kPileupChannels];
        for (int c = 0; c < kPileupChannels; ++c) m[c] = p.img[i * kPileupChannels + c];
        const PileupSite s = pileup_site(m, p.depth[i], p.ref[i], p.cfg);
        if (f & 2) {
            int64_t cs = p.tile_base[2 * blockIdx.x + 1];
            for (int w = 0; w < wave; ++w) cs += wave_n[1][w];
            cs += __popcll(b & ((1ull << lane) - 1ull));
            ci = (int32_t)cs;
            PileupCandRec rec{};
            rec.pos = p.start + i, rec.depth = s.depth, rec.ref_depth = s.ref_count - s.del_count - s.ins_count;
            for (int c = 0; c < 4; ++c) rec.x[c] = m[c] + m[9 + c];
            rec.ref_base = s.ref_base, rec.r = (uint8_t)s.r;
            p.out_cand[cs] = rec;
            p.out_cpos[cs] = p.start + i, p.out_cdepth[cs] = s.depth;
        }
        m[s.r] = -s.fwd_sum, m[9 + s.r] = -s.rev_sum;
        for (int c = 0; c < kPileupChannels; ++c) p.out_matrix[slot * kPileupChannels + c] = m[c];
        p.out_major[slot] = p.start + i;
    }
    p.cand_index[i] = ci;
}

C3_PILEUP_TEXT __global__ __launch_bounds__(256) void pileup_alleles_kernel(PileupParams p) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= p.cap || p.key[s] == kPileupEmpty) return;
    const int64_t k = p.rep[s];
    const int32_t read = p.op_read[k];
    int64_t col;
    int32_t len;
    if (read < 0 || !pileup_event(p, k, read, &col, &len)) return;
    const int32_t ci = p.cand_index[col];
    if (ci < 0) return;
    const int64_t at = atomicAdd(&p.scalars[3], 1u);
    if (at >= p.allele_cap) return;  // (cannot happen: there are no more records than slots in use, and allele_cap is their bound)
    PileupAlleleRec rec{};
    rec.cand = ci, rec.len = len, rec.read = read, rec.q = p.op_q[k], rec.count = p.cnt[s];
    rec.ins = (int)(p.cigar[k] & 15) == kOpI, rec.rev = (p.flag[read] & 16) ? 1 : 0;
    p.out_allele[at] = rec;
}

}  // namespace c3

// ------------------------------------------------------------------------------------------ the context
struct c3_pileup {
    int device = -1;  // < 0: no GPU behind this context
    hipStream_t stream = nullptr;
    hipEvent_t ev[9] = {};
    hipEvent_t ready = nullptr, taken = nullptr;  // ready: the held device result is complete; taken: the last ring batch has copied it (c3_predict_submit_pileup)
    bool taken_set = false;
    int64_t start = 0, n = 0;  // the region of the held device result
    struct Run { int64_t first, last, col; };  // a stretch of consecutive existing columns: positions, and its first column in the matrix
    std::vector<Run> runs;     // of the held device result, from the sites' existence flags (one byte a site comes back with the totals)
    c3::PileupResult host;  // the held result of the host form; after a device call its text (and nothing else)
    bool on_host = true;
    int64_t n_cols = 0, n_cand = 0, n_sites = 0;  // of the held device result
    c3_pileup_counters stats{};
    struct Buf {
        void *p = nullptr;
        size_t bytes = 0;
    };
    // grown on demand, never shrunk: the read set, per-op arrays, the event table, per-site arrays, per-tile words, the compacted result
    Buf pos, flag, mapq, cfirst, cigar, sfirst, seq, ref, op_rpos, op_q, op_read, ev_slot, key, cnt, rep, img, other, depth, cand_index, span, flags,
        n_ref, n_total, tiles, scalars, out_matrix, out_major, out_cpos, out_cdepth, out_cand, out_allele;
};

namespace c3 {

static int pileup_grow(c3_pileup::Buf &b, size_t bytes) {
    if (bytes <= b.bytes) return 0;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr, b.bytes = 0;
    bytes = std::max<size_t>((bytes + 255) & ~(size_t)255, 256);
    HIP_TRY(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return 0;
}

#define PILEUP_LAUNCH(kernel, grid, block, ...)                                                               \
    do {                                                                                                      \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(block), 0, g->stream, __VA_ARGS__);           \
        HIP_TRY(hipGetLastError());                                                                           \
    } while (0)

static int pileup_held_on_host(c3_pileup *g, const c3_read_set *rs, int64_t start, int64_t end, const uint8_t *ref, int64_t ref_first,
                               const c3_pileup_config &cfg) {
    int64_t events = 0;
    pileup_rule_host(rs, start, end, ref, ref_first, cfg, g->host, &events);
    g->on_host = true, g->stats.on_host = 1, g->stats.events = events;
    return 0;
}

// the lines of a device call: the candidate and allele records, sorted and merged on the host
static void pileup_text_from_records(const c3_read_set *rs, const std::vector<PileupCandRec> &cand, std::vector<PileupAlleleRec> &al, const uint8_t *ref,
                                     int64_t ref_first, int32_t max_indel_length, std::string &text) {
    std::sort(al.begin(), al.end(), [](const PileupAlleleRec &a, const PileupAlleleRec &b) { return a.cand < b.cand; });
    size_t e = 0;
    std::vector<PileupAllele> dels, inss;
    text.clear();
    for (size_t c = 0; c < cand.size(); ++c) {
        dels.clear(), inss.clear();
        for (; e < al.size() && al[e].cand == (int32_t)c; ++e) {
            PileupAllele a;
            a.len = al[e].len, a.count = al[e].count;
            if (al[e].ins) a.bases = pileup_bases(rs, al[e].read, al[e].q, al[e].len);
            (al[e].ins ? inss : dels).push_back(std::move(a));
        }
        pileup_merge_sorted(dels), pileup_merge_sorted(inss);
        const PileupCandRec &r = cand[c];
        pileup_print(text, r.pos, r.depth, r.ref_base, r.r, r.x, dels, inss, r.ref_depth, ref + (r.pos - ref_first), max_indel_length);
    }
}

static int pileup_device(c3_pileup *g, const c3_read_set *rs, int64_t start, int64_t end, const uint8_t *ref, int64_t ref_first, const c3_pileup_config &cfg,
                         const PileupCensus &census) {
    HIP_TRY(hipSetDevice(g->device));
    const int64_t n = end - start, nr = rs->n_reads, n_ops = census.ops;
    const int64_t c_base = nr ? rs->cigar_first[0] : 0, s_base = nr ? rs->seq_first[0] : 0;
    const int64_t seq_bytes = nr ? rs->seq_first[nr] - s_base : 0;
    uint32_t cap = 64;
    while ((int64_t)cap < 2 * census.indel_ops) cap <<= 1;  // (indel_ops <= kPileupMaxIndelOps = 2^29, pileup_check: cap <= 2^30)
    PileupParams p{};
    p.cfg = cfg, p.cfg.hash_mask = cfg.hash_mask ? cfg.hash_mask : ~0ull, p.start = start, p.end = end, p.n = n, p.n_reads = nr, p.n_ops = n_ops, p.cap = cap;
    p.tiles = (n + kPileupTile - 1) / kPileupTile;
    TRY(pileup_grow(g->pos, (size_t)nr * 8));
    TRY(pileup_grow(g->flag, (size_t)nr * 2));
    TRY(pileup_grow(g->mapq, (size_t)nr));
    TRY(pileup_grow(g->cfirst, (size_t)(nr + 1) * 8));
    TRY(pileup_grow(g->sfirst, (size_t)(nr + 1) * 8));
    TRY(pileup_grow(g->cigar, (size_t)n_ops * 4));
    TRY(pileup_grow(g->seq, (size_t)seq_bytes));
    TRY(pileup_grow(g->ref, (size_t)n));
    TRY(pileup_grow(g->op_rpos, (size_t)n_ops * 8));
    TRY(pileup_grow(g->op_q, (size_t)n_ops * 4));
    TRY(pileup_grow(g->op_read, (size_t)n_ops * 4));
    TRY(pileup_grow(g->ev_slot, (size_t)n_ops * 4));
    TRY(pileup_grow(g->key, (size_t)cap * 8));
    TRY(pileup_grow(g->cnt, (size_t)cap * 4));
    TRY(pileup_grow(g->rep, (size_t)cap * 4));
    TRY(pileup_grow(g->img, (size_t)n * kPileupChannels * 4));
    TRY(pileup_grow(g->other, (size_t)n * 4));
    TRY(pileup_grow(g->depth, (size_t)n * 4));
    TRY(pileup_grow(g->cand_index, (size_t)n * 4));
    TRY(pileup_grow(g->span, (size_t)n));
    TRY(pileup_grow(g->flags, (size_t)n));
    TRY(pileup_grow(g->n_ref, (size_t)n * 8));
    TRY(pileup_grow(g->n_total, (size_t)n * 8));
    TRY(pileup_grow(g->tiles, (size_t)(4 * p.tiles + 2) * 4));
    TRY(pileup_grow(g->scalars, 64));
    p.pos = (const int64_t *)g->pos.p, p.flag = (const uint16_t *)g->flag.p, p.mapq = (const uint8_t *)g->mapq.p;
    p.cigar_first = (const int64_t *)g->cfirst.p, p.seq_first = (const int64_t *)g->sfirst.p, p.cigar = (const uint32_t *)g->cigar.p;
    p.seq = (const uint8_t *)g->seq.p, p.ref = (const uint8_t *)g->ref.p;
    p.op_rpos = (int64_t *)g->op_rpos.p, p.op_q = (int32_t *)g->op_q.p, p.op_read = (int32_t *)g->op_read.p, p.ev_slot = (int32_t *)g->ev_slot.p;
    p.key = (uint64_t *)g->key.p, p.cnt = (uint32_t *)g->cnt.p, p.rep = (uint32_t *)g->rep.p;
    p.img = (int32_t *)g->img.p, p.other = (int32_t *)g->other.p, p.depth = (int32_t *)g->depth.p, p.cand_index = (int32_t *)g->cand_index.p;
    p.span = (uint8_t *)g->span.p, p.flags = (uint8_t *)g->flags.p, p.n_ref = (int64_t *)g->n_ref.p, p.n_total = (int64_t *)g->n_total.p;
    p.tile_n = (uint32_t *)g->tiles.p, p.tile_base = p.tile_n + 2 * p.tiles, p.scalars = (uint32_t *)g->scalars.p;

    hipStream_t st = g->stream;
    if (g->taken_set) HIP_TRY(hipStreamWaitEvent(st, g->taken, 0));  // a ring batch may still be copying the result this call overwrites
    g->taken_set = false;
    HIP_TRY(hipEventRecord(g->ev[0], st));
    // the read set, staged once; the offset tables rebased to the first read's (the kernels index the staged arrays from 0)
    if (nr > 0) {
        std::vector<int64_t> cf((size_t)nr + 1), sf((size_t)nr + 1);
        for (int64_t r = 0; r <= nr; ++r) cf[(size_t)r] = rs->cigar_first[r] - c_base, sf[(size_t)r] = rs->seq_first[r] - s_base;
        TRY(h2d_staged(g->pos.p, rs->pos, (size_t)nr * 8, st));
        TRY(h2d_staged(g->flag.p, rs->flag, (size_t)nr * 2, st));
        TRY(h2d_staged(g->mapq.p, rs->mapq, (size_t)nr, st));
        TRY(h2d_staged(g->cfirst.p, cf.data(), (size_t)(nr + 1) * 8, st));
        TRY(h2d_staged(g->sfirst.p, sf.data(), (size_t)(nr + 1) * 8, st));
        if (n_ops) TRY(h2d_staged(g->cigar.p, rs->cigar + c_base, (size_t)n_ops * 4, st));
        if (seq_bytes) TRY(h2d_staged(g->seq.p, rs->seq + s_base, (size_t)seq_bytes, st));
    }
    TRY(h2d_staged(g->ref.p, ref + (start - ref_first), (size_t)n, st));
    HIP_TRY(hipMemsetAsync(g->img.p, 0, (size_t)n * kPileupChannels * 4, st));
    HIP_TRY(hipMemsetAsync(g->other.p, 0, (size_t)n * 4, st));
    HIP_TRY(hipMemsetAsync(g->span.p, 0, (size_t)n, st));
    HIP_TRY(hipMemsetAsync(g->key.p, 0xff, (size_t)cap * 8, st));
    HIP_TRY(hipMemsetAsync(g->cnt.p, 0, (size_t)cap * 4, st));
    HIP_TRY(hipMemsetAsync(g->scalars.p, 0, 64, st));
    HIP_TRY(hipEventRecord(g->ev[1], st));
    const int64_t grid_ops = (n_ops + 255) / 256, grid_n = (n + 255) / 256, grid_cap = ((int64_t)cap + 255) / 256;
    if (nr > 0) PILEUP_LAUNCH(pileup_ops_kernel, (nr + 3) / 4, 256, p);
    HIP_TRY(hipEventRecord(g->ev[2], st));
    if (n_ops > 0) PILEUP_LAUNCH(pileup_walk_kernel, grid_ops, 256, p);
    HIP_TRY(hipEventRecord(g->ev[3], st));
    if (n_ops > 0) PILEUP_LAUNCH(pileup_verify_kernel, grid_ops, 256, p);
    HIP_TRY(hipEventRecord(g->ev[4], st));
    PILEUP_LAUNCH(pileup_reduce_kernel, grid_cap, 256, p);
    HIP_TRY(hipEventRecord(g->ev[5], st));
    PILEUP_LAUNCH(pileup_exist_kernel, grid_n, 256, p);
    PILEUP_LAUNCH(pileup_site_kernel, grid_n, 256, p);
    HIP_TRY(hipEventRecord(g->ev[6], st));
    PILEUP_LAUNCH(pileup_count_kernel, p.tiles, kPileupTile, p);
    PILEUP_LAUNCH(pileup_scan_kernel, 1, kPileupTile, p);
    uint32_t sc[8] = {}, totals[2] = {};
    TRY(d2h_staged(sc, p.scalars, sizeof(sc), st));
    TRY(d2h_staged(totals, p.tile_base + 2 * p.tiles, sizeof(totals), st));
    g->stats.events = sc[2], g->stats.collisions = sc[1];
    if (sc[4]) return fail("c3_pileup_reads: the event table of %u slots overflowed (%lld I and D ops counted)", cap, (long long)census.indel_ops);
    if (sc[0]) {  // two different events under one key: the host form answers
        g->stats.fell_back = 1;
        return pileup_held_on_host(g, rs, start, end, ref, ref_first, cfg);
    }
    const int64_t n_cols = totals[0], n_cand = totals[1];
    // the stretches of consecutive columns, for the chunk table of the chained entry: its submit then has nothing to fetch
    {
        std::vector<uint8_t> flags((size_t)n);
        TRY(d2h_staged(flags.data(), p.flags, (size_t)n, st));
        g->runs.clear();
        int64_t c = 0, prev = -2;
        for (int64_t i = 0; i < n; ++i) {
            if (!(flags[(size_t)i] & 1)) continue;
            if (i != prev + 1) g->runs.push_back(c3_pileup::Run{start + i, start + i, c});
            else g->runs.back().last = start + i;
            prev = i, ++c;
        }
        if (c != n_cols) return fail("internal: %lld existence flags for %lld columns", (long long)c, (long long)n_cols);
    }
    const int64_t allele_cap = std::max<int64_t>(1, std::min<int64_t>((int64_t)sc[2], (int64_t)cap));
    TRY(pileup_grow(g->out_matrix, (size_t)n_cols * kPileupChannels * 4));
    TRY(pileup_grow(g->out_major, (size_t)n_cols * 8));
    TRY(pileup_grow(g->out_cpos, (size_t)n_cand * 8));
    TRY(pileup_grow(g->out_cdepth, (size_t)n_cand * 4));
    TRY(pileup_grow(g->out_cand, (size_t)n_cand * sizeof(PileupCandRec)));
    TRY(pileup_grow(g->out_allele, (size_t)allele_cap * sizeof(PileupAlleleRec)));
    p.out_matrix = (int32_t *)g->out_matrix.p, p.out_major = (int64_t *)g->out_major.p, p.out_cpos = (int64_t *)g->out_cpos.p;
    p.out_cdepth = (int32_t *)g->out_cdepth.p, p.out_cand = (PileupCandRec *)g->out_cand.p, p.out_allele = (PileupAlleleRec *)g->out_allele.p;
    p.allele_cap = allele_cap;
    PILEUP_LAUNCH(pileup_emit_kernel, p.tiles, kPileupTile, p);
    if (n_cand > 0) PILEUP_LAUNCH(pileup_alleles_kernel, grid_cap, 256, p);
    HIP_TRY(hipEventRecord(g->ev[7], st));
    std::vector<PileupCandRec> cand((size_t)n_cand);
    std::vector<PileupAlleleRec> alleles;
    if (n_cand > 0) {
        uint32_t n_al = 0;
        TRY(d2h_staged(&n_al, p.scalars + 3, 4, st));
        if ((int64_t)n_al > allele_cap) return fail("c3_pileup_reads: %u allele records for %lld slots in use", n_al, (long long)allele_cap);
        alleles.resize(n_al);
        TRY(d2h_staged(cand.data(), p.out_cand, (size_t)n_cand * sizeof(PileupCandRec), st));
        if (n_al) TRY(d2h_staged(alleles.data(), p.out_allele, (size_t)n_al * sizeof(PileupAlleleRec), st));
    }
    HIP_TRY(hipEventRecord(g->ev[8], st));
    HIP_TRY(hipEventRecord(g->ready, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->host.clear();
    pileup_text_from_records(rs, cand, alleles, ref, ref_first, cfg.max_indel_length, g->host.text);
    // the candidates' positions and depths are on the host anyway (their records were fetched for the text): the chained entry stages them
    g->host.cand_pos.resize((size_t)n_cand), g->host.cand_depth.resize((size_t)n_cand);
    for (int64_t c = 0; c < n_cand; ++c) g->host.cand_pos[(size_t)c] = cand[(size_t)c].pos, g->host.cand_depth[(size_t)c] = cand[(size_t)c].depth;
    g->on_host = false, g->n_cols = n_cols, g->n_cand = n_cand, g->n_sites = cfg.gvcf ? n : 0, g->start = start, g->n = n;
    for (int k = 0; k < 8; ++k) {
        float ms = 0;
        // order of ev: 0 start, 1 staged, 2 ops, 3 walk, 4 verify, 5 reduce, 6 site, 7 compaction, 8 records fetched
        static const int slot_of[8] = {6, 0, 1, 2, 3, 4, 5, 7};  // kernel_ms: op table, walk, indel table, reduce, site, compaction, staging, fetch
        HIP_TRY(hipEventElapsedTime(&ms, g->ev[k], g->ev[k + 1]));
        g->stats.kernel_ms[slot_of[k]] = ms;
    }
    return 0;
}

static int pileup_entry(c3_pileup *g, const c3_read_set *rs, int64_t start, int64_t end, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                        const c3_pileup_config *cfg, bool device, const char *what) {
    if (!g) return fail("%s: null context", what);
    if (device && g->device < 0) return fail("%s: this context was created without a device (c3_pileup_reads_host needs none)", what);
    PileupCensus census;
    TRY(pileup_check(rs, start, end, ref_bytes, ref_first, ref_len, cfg, &census));
    g->stats = c3_pileup_counters{};
    g->stats.reads_kept = census.kept, g->stats.reads_dropped = census.dropped;
    // whatever happens below, the context holds no stale result
    g->host.clear(), g->on_host = true, g->n_cols = g->n_cand = g->n_sites = 0;
    if (!device) return pileup_held_on_host(g, rs, start, end, (const uint8_t *)ref_bytes, ref_first, *cfg);
    return pileup_device(g, rs, start, end, (const uint8_t *)ref_bytes, ref_first, *cfg, census);
}

}  // namespace c3

extern "C" {

c3_pileup *c3_pileup_create(int device) {
    using namespace c3;
    c3_pileup *g = new c3_pileup();
    if (device < 0) return g;
    const int ndev = c3_device_count();
    bool ok = false;
    if (ndev <= 0) fail("c3_pileup_create: no HIP device visible (a context with device < 0 and c3_pileup_reads_host need none)");
    else if (device >= ndev) fail("c3_pileup_create: device %d out of range (%d visible)", device, ndev);
    else if (hipSetDevice(device) != hipSuccess) fail("hipSetDevice(%d) failed", device);
    else if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) fail("c3_pileup_create: hipStreamCreate failed");
    else {
        ok = true;
        for (hipEvent_t &e : g->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&g->ready, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&g->taken, hipEventDisableTiming) == hipSuccess;
        if (!ok) fail("c3_pileup_create: hipEventCreate failed");
    }
    if (!ok) {
        for (hipEvent_t e : g->ev)
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

int c3_pileup_destroy(c3_pileup *g) {
    if (!g) return 0;
    if (g->device >= 0) {
        (void)hipSetDevice(g->device);
        if (g->stream) (void)hipStreamSynchronize(g->stream), (void)hipStreamDestroy(g->stream);
        for (hipEvent_t e : g->ev)
            if (e) (void)hipEventDestroy(e);
        if (g->ready) (void)hipEventDestroy(g->ready);
        if (g->taken) (void)hipEventDestroy(g->taken);
        for (c3_pileup::Buf *b : {&g->pos, &g->flag, &g->mapq, &g->cfirst, &g->cigar, &g->sfirst, &g->seq, &g->ref, &g->op_rpos, &g->op_q, &g->op_read,
                                  &g->ev_slot, &g->key, &g->cnt, &g->rep, &g->img, &g->other, &g->depth, &g->cand_index, &g->span, &g->flags, &g->n_ref,
                                  &g->n_total, &g->tiles, &g->scalars, &g->out_matrix, &g->out_major, &g->out_cpos, &g->out_cdepth, &g->out_cand,
                                  &g->out_allele})
            if (b->p) (void)hipFree(b->p);
    }
    delete g;
    return 0;
}

int c3_pileup_reads(c3_pileup *g, const c3_read_set *reads, int64_t start, int64_t end, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                    const c3_pileup_config *cfg) {
    return c3::pileup_entry(g, reads, start, end, ref_bytes, ref_first, ref_len, cfg, true, "c3_pileup_reads");
}

int c3_pileup_reads_host(c3_pileup *g, const c3_read_set *reads, int64_t start, int64_t end, const void *ref_bytes, int64_t ref_first, int64_t ref_len,
                         const c3_pileup_config *cfg) {
    return c3::pileup_entry(g, reads, start, end, ref_bytes, ref_first, ref_len, cfg, false, "c3_pileup_reads_host");
}

int c3_pileup_sizes(c3_pileup *g, int64_t *n_cols, int64_t *n_cand, int64_t *n_sites, int64_t *text_bytes) {
    if (!g) return fail("c3_pileup_sizes: null context");
    if (n_cols) *n_cols = g->on_host ? (int64_t)g->host.major.size() : g->n_cols;
    if (n_cand) *n_cand = g->on_host ? (int64_t)g->host.cand_pos.size() : g->n_cand;
    if (n_sites) *n_sites = g->on_host ? g->host.n_sites : g->n_sites;
    if (text_bytes) *text_bytes = (int64_t)g->host.text.size();
    return 0;
}

int c3_pileup_result(c3_pileup *g, int32_t *matrix, int64_t *major, int64_t *cand_pos, int32_t *cand_depth, int64_t *n_ref, int64_t *n_total,
                     char *text) {
    using namespace c3;
    if (!g) return fail("c3_pileup_result: null context");
    if (text && !g->host.text.empty()) memcpy(text, g->host.text.data(), g->host.text.size());
    auto copy = [](void *dst, const void *src, size_t bytes) {
        if (dst && bytes) memcpy(dst, src, bytes);
    };
    if (g->on_host) {
        const PileupResult &h = g->host;
        copy(matrix, h.matrix.data(), h.matrix.size() * 4), copy(major, h.major.data(), h.major.size() * 8);
        copy(cand_pos, h.cand_pos.data(), h.cand_pos.size() * 8), copy(cand_depth, h.cand_depth.data(), h.cand_depth.size() * 4);
        copy(n_ref, h.n_ref.data(), h.n_ref.size() * 8), copy(n_total, h.n_total.data(), h.n_total.size() * 8);
        return 0;
    }
    HIP_TRY(hipSetDevice(g->device));
    if (matrix && g->n_cols) TRY(d2h_staged(matrix, g->out_matrix.p, (size_t)g->n_cols * kPileupChannels * 4, g->stream));
    if (major && g->n_cols) TRY(d2h_staged(major, g->out_major.p, (size_t)g->n_cols * 8, g->stream));
    if (cand_pos && g->n_cand) TRY(d2h_staged(cand_pos, g->out_cpos.p, (size_t)g->n_cand * 8, g->stream));
    if (cand_depth && g->n_cand) TRY(d2h_staged(cand_depth, g->out_cdepth.p, (size_t)g->n_cand * 4, g->stream));
    if (n_ref && g->n_sites) TRY(d2h_staged(n_ref, g->n_ref.p, (size_t)g->n_sites * 8, g->stream));
    if (n_total && g->n_sites) TRY(d2h_staged(n_total, g->n_total.p, (size_t)g->n_sites * 8, g->stream));
    return 0;
}

// ---- the chained entry: the held result as a candidate batch of the ring (c3_hostring.h).  The region matrix goes from the context's buffer to the
// slot by device-to-device copies on the lane's stream, and the submit waits for nothing.  The candidates' positions and depths are staged
// from the host copy the context holds (they came back with the records for the text): the ring's own host logic reads the depths -- whether
// any window is deep enough to be rescaled decides what is staged, c3_predict_wait counts the rescaled among the kept -- so a device-only
// copy would have to come back first.  The chunk table is the context's list of column stretches, made when the call was.
// From there on the batch is a batch of c3_predict_submit_candidates.  A held result of the host form goes through that entry itself
int c3_predict_submit_pileup(c3_model *m, c3_pileup *g, int head_tail, float *y_host, uint8_t *status_host, int64_t *n_rows_host, int slot) {
    using namespace c3;
    TRY(ring_ready(m, slot));
    if (!g) return fail("c3_predict_submit_pileup: null pileup context");
    if (m->kind != C3_KIND_PILEUP) return fail("candidate selection needs a pileup model: a full-alignment handle has no region matrix");
    if (!n_rows_host) return fail("null buffer: n_rows_host");
    if (g->on_host) {
        const PileupResult &h = g->host;
        return c3_predict_submit_candidates(m, h.matrix.data(), C3_DTYPE_I32, (int64_t)h.major.size(), h.major.data(), h.cand_pos.data(), h.cand_depth.data(),
                                            (int64_t)h.cand_pos.size(), head_tail, y_host, status_host, n_rows_host, slot);
    }
    if (g->device != m->device) return fail("c3_predict_submit_pileup: the pileup context is on device %d, the model on device %d", g->device, m->device);
    const int64_t n_cand = g->n_cand, n_cols = g->n_cols;
    if (n_cand > 0 && (!y_host || !status_host)) return fail("null buffer: rows / status");
    HIP_TRY(hipSetDevice(g->device));
    CandInput ci;
    ci.pos = g->host.cand_pos.data(), ci.head_tail = head_tail != 0, ci.status_host = status_host, ci.n_rows_host = n_rows_host;
    ci.dev_image = g->out_matrix.p, ci.dev_ready = g->ready, ci.dev_taken = g->taken;
    const int64_t pad = ci.head_tail ? m->positions - 1 : 0;
    for (size_t k = 0; k < g->runs.size(); ++k) {
        ci.chunks.push_back(SelectChunk{g->runs[k].first, g->runs[k].last, g->runs[k].col + (2 * (int64_t)k + 1) * pad});
        ci.src_col.push_back(g->runs[k].col);
    }
    const int64_t img_cols = n_cols + 2 * pad * (int64_t)ci.chunks.size();
    if (img_cols > INT32_MAX - m->positions) return fail("region too large: %lld columns on the device", (long long)img_cols);
    if (n_cand > 0) TRY(depth_args_ok(m, C3_DTYPE_I32, n_cand, g->host.cand_depth.data(), true));
    RingInput in = ring_input(InKind::Candidates, g->out_matrix.p, C3_DTYPE_I32, n_cand, y_host, n_cand ? g->host.cand_depth.data() : nullptr);
    in.n_cols = img_cols, in.cand = &ci;
    if (n_cand == 0 || img_cols < m->positions) {  // (as c3_predict_submit_candidates: nothing to launch)
        verify_count(m, n_cand, false);
        record_batch(m, m->slot[slot], in, StagedBatch(), -1, false);
        return 0;
    }
    g->taken_set = true;  // (queue_device_image records it behind its copies, in front of the forward pass; set first: a submit that fails
    return predict_submit(m, in, slot);  // behind them leaves the event recorded)
}

int c3_predict_pileup_reads(c3_model *m, c3_pileup *g, int head_tail, float *y_host, uint8_t *status_host, int64_t *n_rows_host) {
    TRY(c3_predict_submit_pileup(m, g, head_tail, y_host, status_host, n_rows_host, 0));
    return c3_predict_wait(m, 0);
}

int c3_pileup_stats(c3_pileup *g, c3_pileup_counters *out) {
    if (!g || !out) return fail("c3_pileup_stats: null argument");
    *out = g->stats;
    return 0;
}

int c3_pileup_tile_sites(void) { return c3::kPileupTile; }

}  // extern "C"
