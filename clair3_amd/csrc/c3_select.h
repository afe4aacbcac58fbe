// c3_select.h -- which windows of a pileup region the reference would have fed the model, decided on the device from candidate POSITIONS
// (preprocess/CreateTensorPileupFromCffi.py:343-397, the loop over all_alt_info_list; __enforce_pileup_chunk_contiguity :180-236).
//
// The rule (F = flanking bases = (positions - 1) / 2 = 16; a chunk is a maximal run of `major` with steps of exactly 1, first / last its
// first and last major; a candidate belongs to the one chunk with first <= pos <= last):
//   * its window covers positions pos - F - 1 .. pos + F - 1 (the reference's `offset = start - first - 1` with start = pos - F: the window is
//     NOT centred on pos, and that is what the network was trained on);
//   * main  (pos - F - 1 >= first and pos + F + 1 <= last): 33 in-chunk columns; dropped when one of them is all zero over its C counts;
//   * with head_tail (--enable_variant_calling_at_sequence_head_and_tail), only where the main test failed:
//       pos - F - 1 < first: kept iff the window's last position pos + F - 1 <= last; the columns before `first` are zero rows (head);
//       else (pos + F + 1 > last): always kept; the columns after `last` are zero rows (tail).  Not tested for empty columns;
//   * everything else: no window.
// Zero rows without touching the kernels that read windows: with head_tail the host lays the device image out chunk by chunk with
// positions - 1 zero columns in front of and behind each chunk (c3_hostring.h), so a padded window is an ordinary in-range start column.
//
// Three launches on the batch's stream, in front of the unchanged forward pass:
//   candidate_status_kernel    one wave per candidate: chunk lookup (binary search in the chunk table the host built from `major`), the rule ->
//                              status byte and start column; lane t tests column t of a main window: all C counts zero?  (The other form of
//                              that test -- one pass over the image that leaves a flag per column, the waves then reading 33 flags -- was
//                              measured beside this one and lost by 6 - 7 %, with one launch and one buffer more:
//                              profiles/candidates_select.txt.  Neighbouring candidates share their columns' cache lines.)
//   kept_count_kernel + compact_kept_kernel   order-preserving compaction of (start, depth) of the kept candidates to the front: ballots
//                              inside a wave, a fixed-order scan over the waves of a workgroup and over the workgroups' counts.  No atomics:
//                              the result does not depend on scheduling.  The remainder is filled with start 0 / depth 0 (an in-range window
//                              whose row nobody reads) and the count goes to a device word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

// (the values of C3_CAND_* in include/c3hip.h)
enum : uint8_t { kCandNoWindow = 0, kCandMain = 1, kCandEmptyColumn = 2, kCandHead = 3, kCandTail = 4 };

struct SelectChunk {
    int64_t first, last;  // major of the chunk's first and last column
    int64_t col;          // column of `first` in the device image
};

struct SelectParams {
    const int32_t *x;           // device image [img_cols][C]
    const SelectChunk *chunks;  // [n_chunks], ascending
    const int64_t *pos;         // [n_cand]
    const int32_t *depth_in;    // [n_cand] or nullptr
    uint8_t *status;            // [n_cand]
    int32_t *start_all;         // [n_cand] start column of every candidate (0 where it has no window)
    int32_t *starts;            // [n_cand] compacted
    int32_t *depth;             // [n_cand] compacted, or nullptr
    uint32_t *block_kept;       // [ceil(n_cand / kCompactTile)]
    uint32_t *n_rows;           // one word
    int n_cand, n_chunks, C, T, head_tail;
    int64_t img_cols;
};

constexpr int kSelectThreads = 256;   // four candidates (waves) per workgroup
constexpr int kCompactTile = 1024;    // candidates per workgroup of the compaction: 16 waves

// V = 2: int2 loads (C even: a column of C counts starts at a multiple of 8 bytes)
template <int V>
__device__ __forceinline__ bool column_is_empty(const int32_t *col, int C) {
    int32_t any = 0;
    if constexpr (V == 2) {
        const int2 *c2 = reinterpret_cast<const int2 *>(col);
        for (int i = 0; i < C / 2; ++i) {
            const int2 v = c2[i];
            any |= v.x | v.y;
        }
    } else {
        for (int i = 0; i < C; ++i) any |= col[i];
    }
    return any == 0;
}

template <int V>
__global__ __launch_bounds__(kSelectThreads) void candidate_status_kernel(SelectParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kSelectThreads / 64) + (threadIdx.x >> 6);
    if (i >= p.n_cand) return;  // (wave-uniform)
    const int64_t pos = p.pos[i];
    // the last chunk with first <= pos
    int lo = 0, hi = p.n_chunks;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.chunks[mid].first <= pos) lo = mid + 1;
        else hi = mid;
    }
    uint8_t st = kCandNoWindow;
    int64_t start = 0;
    if (lo > 0) {
        const SelectChunk ch = p.chunks[lo - 1];
        const int F = (p.T - 1) / 2;
        const int64_t w0 = pos - F - 1, w1 = w0 + p.T - 1;  // positions the window covers
        if (pos <= ch.last) {
            const bool main = w0 >= ch.first && pos + F + 1 <= ch.last;
            if (main) st = kCandMain;
            else if (p.head_tail) {
                if (w0 < ch.first) st = w1 <= ch.last ? kCandHead : kCandNoWindow;
                else st = kCandTail;
            }
            if (st != kCandNoWindow) start = ch.col + (w0 - ch.first);
        }
    }
    // (wave-uniform so far.)  A window can only start inside the image: the host sized it; a start outside would be a bug there, and
    // is turned into "no window" rather than into a read beyond the buffer
    if (st != kCandNoWindow && (start < 0 || start + p.T > p.img_cols)) st = kCandNoWindow, start = 0;
    if (st == kCandMain) {
        bool empty = false;
        for (int t = lane; t < p.T; t += 64) empty |= column_is_empty<V>(p.x + (start + t) * p.C, p.C);
        if (__ballot(empty) != 0ull) st = kCandEmptyColumn;
    }
    if (lane == 0) {
        p.status[i] = st;
        p.start_all[i] = (st == kCandMain || st == kCandHead || st == kCandTail) ? (int32_t)start : 0;
    }
}

__device__ __forceinline__ bool cand_kept(uint8_t st) { return st == kCandMain || st == kCandHead || st == kCandTail; }

// kept candidates of each tile of kCompactTile
__global__ __launch_bounds__(kCompactTile) void kept_count_kernel(SelectParams p) {
    __shared__ uint32_t wave_n[kCompactTile / 64];
    const int i = blockIdx.x * kCompactTile + threadIdx.x;
    const bool keep = i < p.n_cand && cand_kept(p.status[i]);
    const uint64_t b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kCompactTile / 64; ++w) s += wave_n[w];
        p.block_kept[blockIdx.x] = s;
    }
}

// kept candidate i goes to slot (kept before its tile) + (kept before its wave in the tile) + (kept before its lane in the wave); the
// slots from the total on are filled.  Every thread writes only slots of its own: no two writers per word.
__global__ __launch_bounds__(kCompactTile) void compact_kept_kernel(SelectParams p) {
    __shared__ uint32_t wave_n[kCompactTile / 64];
    __shared__ uint32_t part[kCompactTile / 64];
    __shared__ uint32_t base_total[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_tiles = gridDim.x;
    // the counts of all tiles, summed in a fixed order: before this tile, and all
    uint32_t before = 0, all = 0;
    for (int t = tid; t < n_tiles; t += kCompactTile) {
        const uint32_t v = p.block_kept[t];
        all += v;
        if (t < (int)blockIdx.x) before += v;
    }
    for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off, 64), all += __shfl_down(all, off, 64);
    if (lane == 0) wave_n[wave] = before, part[wave] = all;
    __syncthreads();
    if (tid == 0) {
        uint32_t sb = 0, sa = 0;
        for (int w = 0; w < kCompactTile / 64; ++w) sb += wave_n[w], sa += part[w];
        base_total[0] = sb, base_total[1] = sa;
    }
    __syncthreads();
    const uint32_t base = base_total[0], total = base_total[1];
    const int i = blockIdx.x * kCompactTile + tid;
    const bool keep = i < p.n_cand && cand_kept(p.status[i]);
    const uint64_t b = __ballot(keep);
    __syncthreads();  // (wave_n is written again)
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wave_n[w];
    if (keep) {
        const uint32_t slot = base + wbase + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        p.starts[slot] = p.start_all[i];
        if (p.depth) p.depth[slot] = p.depth_in[i];
    }
    if (i < p.n_cand && (uint32_t)i >= total) {  // the surplus windows: an in-range start, never rescaled
        p.starts[i] = 0;
        if (p.depth) p.depth[i] = 0;
    }
    if (blockIdx.x == 0 && tid == 0) *p.n_rows = total;
}

}  // namespace c3
