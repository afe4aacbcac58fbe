// c3_score.h -- score mode (c3_model_set_score): the focal loss and the arg-max accuracy of labelled windows, evaluated on
// the rows of a batch where they are -- the reference's validation pass (clair3/Train.py:87-107 FocalLoss.forward, :210-257 _run_epoch with
// train=False) without its rows ever crossing PCIe.
//
// Per window and task t (columns (0,21) (21,24) (24,57) (57,90), limited to nout; labels (B, nout) in the row's own column layout, int8 or
// float32), the reference's formula with y general (soft labels work; y enters twice):
//   L_t = sum_c  w_c * y_c * (-ln q_c) * (1 - q_c)^gamma * y_c,   q = min(max(p, 1e-9f), 1.0f) in float32
// (the reference's upper clamp 1 - 1e-9 IS 1.0f in float32: p = 1 gives a zero term, p = 0 gives 20.7233).  A NaN passes the clamp as it
// passes torch.clamp.  Arithmetic: q widened to double, the double library's log (and pow for a gamma other than 2), double products, one
// chain over the task's columns in ascending order -- the oracle's stance (c3_exact.h).  The window's value is rounded once, to the float32
// the caller may ask for; the unrounded double joins the sums.
// Beside it per task: the windows whose arg-max of p equals the arg-max of y (first maximum by `>` from -inf on: the lowest index on ties, a
// NaN is never a maximum), and per batch the windows that hold a non-finite probability in their first nout columns -- such a window is not
// hidden: its loss is reported as it comes out and the count says that it was there.
//
// Two launches on the batch's stream behind whatever pass answers the batch:
//   rows_score_kernel         four lanes per window, one per task; a thread walks its windows in ascending order (grid-stride over groups of
//                             64 windows); butterfly over the 16 quads of a wave (a + b on both partners: every lane holds the same sum),
//                             the four waves through LDS in wave order, one partial per workgroup
//   rows_score_final_kernel   one wave: lane k folds quantity k of the workgroups' partials in block order and writes its field of the
//                             batch's ScoreRecord into the slot's output buffer
// No atomics; the grid is a function of the batch size alone, so the record of a batch does not depend on slot, lane or scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace c3 {

constexpr int kScoreThreads = 256;          // 64 windows per workgroup and pass
constexpr int kScoreMaxBlocks = 1024;       // partials of one batch (a larger batch: every workgroup takes several groups), as kVerifyMaxBlocks
constexpr size_t kScoreRecordBytes = 256;   // the record's section of a staged batch (a multiple of 256 like every section)
constexpr int kScoreWords = 9;              // 8-byte words of a partial: loss_sum[4] (double), correct[4], nonfinite (int64)
constexpr size_t kScorePartBytes = (size_t)kScoreWords * kScoreMaxBlocks * 8;  // word k of workgroup b lives at part[k * kScoreMaxBlocks + b]
constexpr int kScoreMaxCols = 90;

struct ScoreRecord {  // the batch's record as c3_score_wait reads it
    int32_t windows, tasks;
    double loss_sum[4];  // per task: the sum of the windows' unrounded values
    int64_t correct[4];  // per task: windows whose arg-max of p is the arg-max of y
    int64_t nonfinite;   // windows with a probability that is not finite
};

struct ScoreParams {
    const float *rows;   // [batch][stride], the first nout columns are scored
    const void *labels;  // [batch][nout] int8 or float32
    float *loss;         // [batch][tasks], or nullptr: nobody asked for the windows' values
    uint64_t *part;      // [kScoreWords][kScoreMaxBlocks]
    double gamma;
    int stride, nout, tasks, batch;
    int label_f32, weighted;
    float w[kScoreMaxCols];  // class weights in the row's column layout (weighted != 0)
};

#define C3_SCORE_TEXT __attribute__((section(".c3_score_text")))  // behind `.text`, like the verify kernels: no other kernel moves

__global__ __launch_bounds__(kScoreThreads) C3_SCORE_TEXT void rows_score_kernel(ScoreParams p) {
    __shared__ double wave_loss[kScoreThreads / 64][4];
    __shared__ uint32_t wave_correct[kScoreThreads / 64][4], wave_nonfinite[kScoreThreads / 64];
    const int tid = threadIdx.x, h = tid & 3, lane = tid & 63;
    const int lo = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
    const int hi = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
    const bool g2 = p.gamma == 2.0;
    double t_loss = 0.0;
    uint32_t t_correct = 0, t_nonfinite = 0;
    for (int r0 = blockIdx.x * (kScoreThreads / 4); r0 < p.batch; r0 += gridDim.x * (kScoreThreads / 4)) {  // (uniform over the workgroup)
        const int r = r0 + (tid >> 2);
        int bad = 0;
        if (r < p.batch && lo < hi) {
            const float *row = p.rows + (int64_t)r * p.stride;
            const float *yf = reinterpret_cast<const float *>(p.labels) + (int64_t)r * p.nout;
            const int8_t *yb = reinterpret_cast<const int8_t *>(p.labels) + (int64_t)r * p.nout;
            double L = 0.0;
            float pm = -INFINITY, ym = -INFINITY;
            int pi = lo, yi = lo;
            for (int c = lo; c < hi; ++c) {
                const float pv = row[c], yv = p.label_f32 ? yf[c] : (float)yb[c];
                bad |= (__float_as_uint(pv) & 0x7f800000u) == 0x7f800000u;
                const float q = pv < 1e-9f ? 1e-9f : pv > 1.0f ? 1.0f : pv;  // (a NaN stays a NaN)
                const double qd = (double)q, yd = (double)yv, rest = 1.0 - qd;
                const double ce = -yd * log(qd), wt = (g2 ? rest * rest : pow(rest, p.gamma)) * yd;
                double fl = ce * wt;
                if (p.weighted) fl *= (double)p.w[c];
                L += fl;
                if (pv > pm) pm = pv, pi = c;
                if (yv > ym) ym = yv, yi = c;
            }
            if (p.loss) p.loss[(int64_t)r * p.tasks + h] = (float)L;
            t_loss += L, t_correct += pi == yi;
        }
        // a non-finite probability anywhere in the window (the quad's lanes all have the same r)
        bad |= __shfl_xor(bad, 1, 64);
        bad |= __shfl_xor(bad, 2, 64);
        if (h == 0 && r < p.batch) t_nonfinite += (uint32_t)bad;
    }
    // the wave: lanes of the same task meet (distances 4 .. 32); the count of non-finite windows lives on the lanes of task 0
    for (int off = 4; off < 64; off <<= 1) {
        t_loss += __shfl_xor(t_loss, off, 64);
        t_correct += __shfl_xor(t_correct, off, 64), t_nonfinite += __shfl_xor(t_nonfinite, off, 64);
    }
    if (lane < 4) {
        wave_loss[tid >> 6][lane] = t_loss, wave_correct[tid >> 6][lane] = t_correct;
        if (lane == 0) wave_nonfinite[tid >> 6] = t_nonfinite;
    }
    __syncthreads();
    if (tid < kScoreWords) {  // thread k: word k of the partial, the waves in wave order
        uint64_t word;
        if (tid < 4) {
            double s = wave_loss[0][tid];
            for (int w = 1; w < kScoreThreads / 64; ++w) s += wave_loss[w][tid];
            word = (uint64_t)__double_as_longlong(s);
        } else {
            uint64_t n = 0;
            for (int w = 0; w < kScoreThreads / 64; ++w) n += tid < 8 ? wave_correct[w][tid - 4] : wave_nonfinite[w];
            word = n;
        }
        p.part[(size_t)tid * kScoreMaxBlocks + blockIdx.x] = word;
    }
}

// one wave: the partials of n_parts workgroups -> the batch's record.  Lane k < 9 folds word k in block order and writes its own field
__global__ __launch_bounds__(64) C3_SCORE_TEXT void rows_score_final_kernel(const uint64_t *part, int n_parts, int batch, int tasks, ScoreRecord *out) {
    const int k = threadIdx.x;
    if (k < 4) {
        double s = 0.0;
        for (int i = 0; i < n_parts; ++i) s += __longlong_as_double((long long)part[(size_t)k * kScoreMaxBlocks + i]);
        out->loss_sum[k] = s;
    } else if (k < kScoreWords) {
        uint64_t n = 0;
        for (int i = 0; i < n_parts; ++i) n += part[(size_t)k * kScoreMaxBlocks + i];
        if (k < 8) out->correct[k - 4] = (int64_t)n;
        else out->nonfinite = (int64_t)n;
    } else if (k == kScoreWords) out->windows = batch, out->tasks = tasks;
}

static inline int score_blocks(int64_t batch) {
    return (int)std::min<int64_t>(kScoreMaxBlocks, (batch + kScoreThreads / 4 - 1) / (kScoreThreads / 4));
}

}  // namespace c3
