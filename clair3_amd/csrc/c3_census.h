// c3_census.h -- the census of score mode (c3_model_set_score_census): per task a confusion table, a reliability table and
// counts of windows whose two best probabilities lie close together, counted on the rows of a scored batch where they are.  It replaces
// asking for every row (96 - 360 B per window across PCIe) and counting in numpy; the reference has nothing of the kind
// (clair3/Train.py:210-257 returns a loss).  The rule in numpy: synthetic.score_census.
//
// THE definitions (the numpy rule, include/c3hip.h and the kernel below cite this block; tests/test_score_census.py reads it):
//   kScoreCensusBins = 20          reliability bins over [0, 1]: b = min(19, (int)(conf * 20.0f)), the product in float32
//   kScoreCensusGaps = 6           thresholds of the gap counts, float32: 1e-6 1e-5 1e-4 1e-3 1e-2 1e-1 (score_census_gap_thr)
//   kScoreCensusConfUnit = 2^32    fixed-point unit of the confidence sums: exact for conf >= 2^-9, and 2e9 windows fit one bin
//   kScoreCensusCells = 2628       confusion cells: 21^2 + 3^2 + 33^2 + 33^2, task t from kScoreCensusCellOff[t], [truth][pred]
// Per window and task t (columns as in c3_score.h, limited to nout; probabilities float32 as they come out, not clamped):
//   pred / truth   arg-max of p / of y by the rule of c3_score.h -- first maximum by `>` from -inf on, lowest index on ties, a NaN never,
//                  an all-NaN head yields index 0: the very indices rows_score_kernel compares for correct[]
//   confusion[truth][pred] += 1 for every window, so sum == windows and trace == correct[t] of the batch's ScoreRecord
//   conf = p[pred] (-inf when the head is all NaN).  Finite and 0 <= conf <= 1: rel_windows[b] += 1, rel_correct[b] += (pred == truth),
//                  rel_conf_q32[b] += (int64)rint((double)conf * 2^32); otherwise rel_skipped += 1
//   second = the maximum by the same rule over the task's columns other than pred; gap = conf - second in float32;
//   gap_below[k] += (gap < thr_k), cumulative; a NaN or infinite gap fails every comparison
//
// One launch on the batch's stream behind the score kernels (a memset of the batch's table in front of it):
//   rows_census_kernel   four lanes per window, one per task, as rows_score_kernel; a workgroup counts its windows (grid-stride over groups of
//                        64) in a table in LDS with LDS atomics and adds the cells that are not zero to the batch's table
// Integers only: any order of the additions gives the same table, so the table of a batch does not depend on slot, lane or scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

constexpr int kScoreCensusBins = 20;
constexpr int kScoreCensusGaps = 6;
constexpr double kScoreCensusConfUnit = 4294967296.0;
constexpr int kScoreCensusCells = 2628;
__host__ __device__ constexpr float score_census_gap_thr(int k) {
    constexpr float thr[kScoreCensusGaps] = {1e-6f, 1e-5f, 1e-4f, 1e-3f, 1e-2f, 1e-1f};
    return thr[k];
}
constexpr int kScoreCensusCellOff[4] = {0, 441, 450, 1539}, kScoreCensusClasses[4] = {21, 3, 33, 33};
constexpr int kScoreCensusThreads = 256;     // 64 windows per workgroup and pass
constexpr int kScoreCensusMaxBlocks = 256;   // a batch of more than 256 * 64 windows: every workgroup takes several groups

// the table of ONE batch as the kernel fills it: 32-bit counts (a batch holds at most 2^30 windows), 64-bit confidence sums
struct ScoreCensusTable {
    uint64_t rel_conf_q32[4][kScoreCensusBins];
    uint32_t confusion[kScoreCensusCells];
    uint32_t rel_windows[4][kScoreCensusBins], rel_correct[4][kScoreCensusBins];
    uint32_t rel_skipped[4];
    uint32_t gap_below[4][kScoreCensusGaps];
};
constexpr int kScoreCensusWords32 = kScoreCensusCells + 2 * 4 * kScoreCensusBins + 4 + 4 * kScoreCensusGaps;  // the 32-bit counters, behind the 64-bit sums
static_assert(sizeof(ScoreCensusTable) == 8 * 4 * kScoreCensusBins + 4 * kScoreCensusWords32, "ScoreCensusTable has no padding");
constexpr size_t kScoreCensusBytes = (sizeof(ScoreCensusTable) + 255) & ~(size_t)255;  // the table's section of a staged batch

struct ScoreCensusParams {
    const float *rows;   // [batch][stride], the first nout columns are counted
    const void *labels;  // [batch][nout] int8 or float32
    ScoreCensusTable *out;    // zero when the kernel starts
    int stride, nout, batch, label_f32;
};

#define C3_CENSUS_TEXT __attribute__((section(".c3_census_text")))  // behind `.c3_score_text`: no other kernel moves

__global__ __launch_bounds__(kScoreCensusThreads) C3_CENSUS_TEXT void rows_census_kernel(ScoreCensusParams p) {
    __shared__ ScoreCensusTable tab;
    uint32_t *const tab32 = tab.confusion;
    uint64_t *const tab64 = &tab.rel_conf_q32[0][0];
    const int tid = threadIdx.x, h = tid & 3;
    for (int i = tid; i < kScoreCensusWords32; i += kScoreCensusThreads) tab32[i] = 0;
    for (int i = tid; i < 4 * kScoreCensusBins; i += kScoreCensusThreads) tab64[i] = 0;
    __syncthreads();
    const int lo = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
    const int hi = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
    const int cell0 = h == 0 ? 0 : h == 1 ? 441 : h == 2 ? 450 : 1539, K = h == 0 ? 21 : h == 1 ? 3 : 33;
    for (int r0 = blockIdx.x * (kScoreCensusThreads / 4); r0 < p.batch; r0 += gridDim.x * (kScoreCensusThreads / 4)) {
        const int r = r0 + (tid >> 2);
        if (r >= p.batch || lo >= hi) continue;
        const float *row = p.rows + (int64_t)r * p.stride;
        const float *yf = reinterpret_cast<const float *>(p.labels) + (int64_t)r * p.nout;
        const int8_t *yb = reinterpret_cast<const int8_t *>(p.labels) + (int64_t)r * p.nout;
        float pm = -INFINITY, ym = -INFINITY;
        int pi = lo, yi = lo;
        for (int c = lo; c < hi; ++c) {  // the arg-max rule of rows_score_kernel, word for word
            const float pv = row[c], yv = p.label_f32 ? yf[c] : (float)yb[c];
            if (pv > pm) pm = pv, pi = c;
            if (yv > ym) ym = yv, yi = c;
        }
        float second = -INFINITY;
        for (int c = lo; c < hi; ++c) {
            const float pv = row[c];
            if (c != pi && pv > second) second = pv;
        }
        const int pred = pi - lo, truth = yi - lo;
        atomicAdd(&tab.confusion[cell0 + truth * K + pred], 1u);
        const float conf = pm;  // p[pred]; -inf when nothing was a maximum
        if (conf >= 0.0f && conf <= 1.0f) {  // (finite: an infinity or a NaN fails one of the two)
            const int b = min(kScoreCensusBins - 1, (int)(conf * (float)kScoreCensusBins));
            atomicAdd(&tab.rel_windows[h][b], 1u);
            if (pred == truth) atomicAdd(&tab.rel_correct[h][b], 1u);
            atomicAdd((unsigned long long *)&tab.rel_conf_q32[h][b], (unsigned long long)(long long)rint((double)conf * kScoreCensusConfUnit));
        } else
            atomicAdd(&tab.rel_skipped[h], 1u);
        const float gap = conf - second;
#pragma unroll
        for (int k = 0; k < kScoreCensusGaps; ++k)
            if (gap < score_census_gap_thr(k)) atomicAdd(&tab.gap_below[h][k], 1u);
    }
    __syncthreads();
    uint32_t *const out32 = p.out->confusion;
    unsigned long long *const out64 = (unsigned long long *)&p.out->rel_conf_q32[0][0];
    for (int i = tid; i < kScoreCensusWords32; i += kScoreCensusThreads)
        if (const uint32_t v = tab32[i]) atomicAdd(&out32[i], v);
    for (int i = tid; i < 4 * kScoreCensusBins; i += kScoreCensusThreads)
        if (const uint64_t v = tab64[i]) atomicAdd(&out64[i], (unsigned long long)v);
}

static inline int score_census_blocks(int64_t batch) {
    return (int)std::min<int64_t>(kScoreCensusMaxBlocks, (batch + kScoreCensusThreads / 4 - 1) / (kScoreCensusThreads / 4));
}

}  // namespace c3
