// c3_exact.h -- the exact form: both networks in fp64 from end to end on the device (c3_predict_exact / c3_exact_fetch),
// and its place on the submit / wait ring: what answers a batch (c3_model_set_answer), what verify mode compares with
// (c3_model_set_verify_reference) and the repair of C3_VERIFY_REPLACE (further down: "the exact form on the ring").
//
// An INSTRUMENT, not a product form: the arithmetic of oracle/c3_oracle.c -- the checkpoint's fp32 weights widened to double, every
// product, sum, activation and intermediate tensor double, exp / tanh / expm1 the double-precision library functions, no channel
// exponent, no weight scale, no calibration lowering, no precision plan -- at the speed of the chip instead of half a second per window.
// BatchNorm is folded into the convolutions on the host in double and never rounded to fp32 (c3_pack.h pack_exact).  Every
// contraction runs on v_mfma_f64_16x16x4_f64, whose lane map differs from every other matrix instruction's:
//     A: lane holds A[row = lane & 15][k = lane >> 4]      B: lane holds B[k = lane >> 4][col = lane & 15]
//     D: register r of a lane holds D[row = (lane >> 4) + 4 r][col = lane & 15]
// Nothing is tuned: tiles go through LDS, one stage, and the reduction over K of an output element is ONE sequential chain (no
// split-K), so a window's row does not depend on the batch or the chunk it travels in.
//
//   exact_gemm_kernel<Loader, EPI>   out[M][N] = epi(A[M][K] . W[N][K]^T): tiles of 64 x 64, K chunks of 16, edge tiles in M, N and K.
//                                    Loaders: ExDense<T> rows of a matrix of double / int8 / int32 (L4, L5, the heads, the LSTM input
//                                    projections over all steps, LSTM1's straight from the windows); ExConv<T, NORM> the implicit 3x3
//                                    convolution, stride 1 or 2, zero padding, on NHWC double or (conv1) on the int8 windows with x / 100,
//                                    any channel count and byte address.  Epilogues: bias | bias, residual, ReLU | bias, SELU
//   exact_lstm_kernel<H>             one workgroup per (16 windows, direction), one wave per 16 units: gates = gx[t] + h . W_hh^T with
//                                    W_hh streamed from L2 in fragment order, c in registers, h in LDS; rows beyond the batch are zero
//                                    and never stored
//   exact_spp_kernel                 PyramidPolling over the bin table of spp_bins (c3_forward.h)
//   exact_softmax_kernel             softmax(selu(logits)) per head, in the oracle's order of operations
//   exact_rows_to_f32_kernel         the ring: the fp64 rows of a pass rounded to float32 into the slot's rows (and kept as doubles for verify mode)
//   rows_compare_f64_kernel, rows_compare_f64_final_kernel, rows_replace_kernel<R>   verify mode against fp64 rows, and C3_VERIFY_REPLACE
// Rows and fetched tensors of the blocking entry leave through the pinned bounce buffer (c3_model.h d2h_staged): their layouts are the host's already.
//
// Workspace (c3_model.h ExactState): separate from the lanes', allocated at the first exact call, grown on demand, freed with the
// handle.  A call is cut into passes of at most C3HIP_EXACT_CHUNK windows (default 256 full alignment, 1024 pileup); every layer output
// of the last pass stays for c3_exact_fetch.  Per window of a pass, doubles: full alignment (89 x 33) 3 x 48960 + 3 x 26496 + 3 x 15360
// activations + 3584 pooled + 256 + 512 + 2 x 90 = 277 140 (2.22 MB) and the int8 window; pileup 33 x (1024 + 256 + 1280 + 320) + 128 +
// 512 + 2 x 90 = 95 860 (0.77 MB) and the window.
#pragma once
#include "c3_forward.h"

namespace c3 {

typedef double ex_f64x4 __attribute__((ext_vector_type(4)));
enum { kExBias = 0, kExBiasResRelu = 1, kExBiasSelu = 2 };
constexpr int kExBM = 64, kExBN = 64, kExBK = 16, kExLd = kExBK + 1;

__device__ inline double ex_selu(double x) {
    return x > 0.0 ? 1.0507009873554804934193349852946 * x
                   : 1.0507009873554804934193349852946 * 1.6732632423543772848170429916717 * expm1(x);
}
__device__ inline double ex_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

struct ExGemm {
    const double *w;     // [N][K]
    const double *bias;  // [N]
    const double *res;   // kExBiasResRelu: [M][ldc] added before the ReLU, or nullptr
    double *out;         // [M][ldc]
    int M, N, K;
    int64_t ldc;
};

// rows of a [M][lda] matrix of T
template <class T>
struct ExDense {
    struct Params { const T *a; int64_t lda; };
    struct Row { const T *p; };
    static __device__ Row row(const Params &p, int m) { return {p.a + (int64_t)m * p.lda}; }
    static __device__ double at(const Params &, const Row &r, int k) { return (double)r.p[k]; }
};
// row m = (window, oh, ow) of the implicit 3x3 convolution, k = (kh * 3 + kw) * C + ci; NORM: the value / 100 (model.py:378)
template <class T, bool NORM>
struct ExConv {
    struct Params { const T *x; int H, W, C, Ho, Wo, stride; };
    struct Row { const T *img; int ih0, iw0; };
    static __device__ Row row(const Params &p, int m) {
        const int b = m / (p.Ho * p.Wo), r = m - b * (p.Ho * p.Wo), oh = r / p.Wo, ow = r - oh * p.Wo;
        return {p.x + (int64_t)b * p.H * p.W * p.C, oh * p.stride - 1, ow * p.stride - 1};
    }
    static __device__ double at(const Params &p, const Row &r, int k) {
        const int tap = k / p.C, ci = k - tap * p.C, kh = tap / 3, kw = tap - 3 * kh;
        const int ih = r.ih0 + kh, iw = r.iw0 + kw;
        if (ih < 0 || ih >= p.H || iw < 0 || iw >= p.W) return 0.0;
        const double v = (double)r.img[((int64_t)ih * p.W + iw) * p.C + ci];
        return NORM ? v / 100.0 : v;
    }
};

template <class L, int EPI>
__global__ __launch_bounds__(256) void exact_gemm_kernel(typename L::Params lp, ExGemm g) {
    __shared__ double As[kExBM][kExLd], Bs[kExBN][kExLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * kExBM, n0 = blockIdx.y * kExBN;
    // staging: thread -> (tile row tid / 4, four consecutive k) of both tiles
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    const bool a_ok = m0 + lr < g.M, b_ok = n0 + lr < g.N;
    const typename L::Row ar = L::row(lp, a_ok ? m0 + lr : 0);
    const double *br = g.w + (int64_t)(b_ok ? n0 + lr : 0) * g.K;
    ex_f64x4 acc[4];
    for (int t = 0; t < 4; ++t) acc[t] = ex_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < g.K; k0 += kExBK) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + lk + j;
            As[lr][lk + j] = a_ok && k < g.K ? L::at(lp, ar, k) : 0.0;
            Bs[lr][lk + j] = b_ok && k < g.K ? br[k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kExBK / 4; ++ks) {
            const double a = As[wave * 16 + (lane & 15)][4 * ks + (lane >> 4)];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[t * 16 + (lane & 15)][4 * ks + (lane >> 4)], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wave * 16 + (lane >> 4) + 4 * r, n = n0 + t * 16 + (lane & 15);
            if (m >= g.M || n >= g.N) continue;
            double v = acc[t][r] + g.bias[n];
            if (EPI == kExBiasResRelu) {
                if (g.res) v += g.res[(int64_t)m * g.ldc + n];
                v = v > 0.0 ? v : 0.0;
            }
            if (EPI == kExBiasSelu) v = ex_selu(v);
            g.out[(int64_t)m * g.ldc + n] = v;
        }
}

// gx [B * T][2 * 4H]: both directions' input projections with both biases, PyTorch gate order i, f, g, o; whh [dir][unit block u][gate]
// [k-step][lane] = W_hh[gate * H + 16 u + (lane & 15)][4 ks + (lane >> 4)]; out [B * T][2H], direction dir at column dir * H
// (clair3/model.py:132-133; torch.nn.LSTM, h0 = c0 = 0; the reverse direction walks t = T - 1 .. 0 and stores h at its own t)
template <int H>
__global__ __launch_bounds__(H / 16 * 64) void exact_lstm_kernel(const double *gx, const double *whh, double *out, int B, int T) {
    constexpr int NU = H / 16, NK = H / 4, LD = H + 1;
    __shared__ double hs[2][16][LD];
    const int dir = blockIdx.y, b0 = blockIdx.x * 16;
    const int tid = threadIdx.x, lane = tid & 63, u = tid >> 6;
    const int col = lane & 15, rq = lane >> 4;
    for (int i = tid; i < 2 * 16 * LD; i += NU * 64) (&hs[0][0][0])[i] = 0.0;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    const double *wf = whh + ((size_t)(dir * NU + u) * 4) * NK * 64 + lane;
    __syncthreads();
    for (int s = 0; s < T; ++s) {
        const int t = dir ? T - 1 - s : s, cur = s & 1;
        ex_f64x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = b0 + rq + 4 * r;
                acc[g][r] = b < B ? gx[((int64_t)b * T + t) * (8 * H) + dir * 4 * H + g * H + u * 16 + col] : 0.0;
            }
#pragma unroll 4
        for (int ks = 0; ks < NK; ++ks) {
            const double a = hs[cur][col][4 * ks + rq];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wf[(size_t)(g * NK + ks) * 64], acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double ig = ex_sigmoid(acc[0][r]), fg = ex_sigmoid(acc[1][r]), gg = tanh(acc[2][r]), og = ex_sigmoid(acc[3][r]);
            c[r] = fg * c[r] + ig * gg;
            const double h = og * tanh(c[r]);
            const int w = rq + 4 * r;
            hs[cur ^ 1][w][u * 16 + col] = h;
            if (b0 + w < B) out[((int64_t)(b0 + w) * T + t) * (2 * H) + dir * H + u * 16 + col] = h;
        }
        __syncthreads();  // (step s + 1 reads hs[cur ^ 1] and writes hs[cur], which every wave has finished reading here)
    }
}

// the bins of p (spp_bins; p.in / p.out unused): out[b][bin][c] = max over the bin's clipped window, 0 taking part where it reached the padding
template <int = 0>  // (templates, like every kernel of this file: instantiated behind the library's other kernels, whose places in the code object stay)
__global__ __launch_bounds__(256) void exact_spp_kernel(SppParams p, const double *in, double *out) {
    const int64_t total = (int64_t)p.B * p.nbins * p.C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % p.C), bin = (int)((i / p.C) % p.nbins);
        const int64_t b = i / ((int64_t)p.C * p.nbins);
        double m = p.pad[bin] ? 0.0 : -1e300;
        for (int h = p.h0[bin]; h < p.h1[bin]; ++h)
            for (int w = p.w0[bin]; w < p.w1[bin]; ++w) {
                const double v = in[((b * p.H + h) * p.W + w) * p.C + c];
                if (v > m) m = v;
            }
        out[i] = m;
    }
}

// y[b][off .. off + n) = softmax(selu(logits[b][off .. off + n))) for each of the nb heads (clair3/model.py:142-150), one thread per (window, head)
template <int = 0>
__global__ __launch_bounds__(256) void exact_softmax_kernel(const double *logits, double *y, int64_t B, int nb, int nout) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * nb) return;
    const int64_t b = i / nb;
    const int br = (int)(i - b * nb);
    const int n = br == 0 ? 21 : br == 1 ? 3 : 33, off = br == 0 ? 0 : br == 1 ? 21 : br == 2 ? 24 : 57;
    const double *lg = logits + b * nout + off;
    double *o = y + b * nout + off;
    double m = -1e300;
    for (int j = 0; j < n; ++j) {
        const double v = ex_selu(lg[j]);
        o[j] = v;
        if (v > m) m = v;
    }
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
        o[j] = exp(o[j] - m);
        s += o[j];
    }
    for (int j = 0; j < n; ++j) o[j] = o[j] / s;
}

// ------------------------------------------------------------------------------------------ the exact form on the ring
// out[b][0 .. nout) = (float)y[b][0 .. nout): the device's conversion, round to nearest even (what numpy's astype(float32) does); out has
// the row stride of the slot's rows (decoder columns behind nout are outcome_maxima_kernel's).  keep: the doubles of the whole batch too
// (verify mode against the exact form compares with them), or nullptr
template <int = 0>
__global__ __launch_bounds__(256) void exact_rows_to_f32_kernel(const double *y, float *out, double *keep, int64_t n, int nout, int stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * nout) return;
    const int64_t b = i / nout;
    const int c = (int)(i - b * nout);
    const double v = y[i];
    out[b * stride + c] = (float)v;
    if (keep) keep[i] = v;
}

// ---- verify mode with the exact rows as the reference (c3_verify.h says what is compared; here b is fp64): |(double)a - b| in double, the
// arg-max and the top-2 gap of b, tol and near_tie as doubles.  The same two launches and the same reduction as rows_compare_kernel /
// rows_compare_final_kernel, the maxima double; the final record is c3_verify.h's VerifyRecord with the maxima rounded to float (round to
// nearest), the double maximum behind it
struct VerifyRecord64 {
    double max_abs;
    double head_max[4];
    uint32_t worst_row, rows_over;
    uint32_t label[4];
    uint32_t tie[4];
};
struct CompareParams64 {
    const float *a;        // the rows under test [batch][stride]
    const double *b;       // the exact rows [batch][nout]
    const uint32_t *kept;  // as CompareParams
    VerifyRecord64 *part;  // [gridDim.x]
    int stride, nout, batch;
    double tol, near_tie;
};
static_assert(sizeof(VerifyRecord) <= kVerifyMax64At && kVerifyReplacedAt + 4 <= kVerifyRecordBytes, "the verify record's section");

__device__ __forceinline__ void verify_max_row64(double &m, uint32_t &row, double om, uint32_t orow) {
    if (om > m || (om == m && orow < row)) m = om, row = orow;
}

template <int = 0>
__global__ __launch_bounds__(kVerifyThreads) void rows_compare_f64_kernel(CompareParams64 p) {
    __shared__ VerifyRecord64 wave_rec[kVerifyThreads / 64];
    const int tid = threadIdx.x, h = tid & 3, lane = tid & 63;
    const int lo = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
    const int hi = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
    const int n = p.kept ? (int)min(*p.kept, (uint32_t)p.batch) : p.batch;
    double t_max = 0.0, t_head = 0.0;
    uint32_t t_row = 0xffffffffu, t_over = 0, t_label = 0, t_tie = 0;
    for (int r0 = blockIdx.x * (kVerifyThreads / 4); r0 < n; r0 += gridDim.x * (kVerifyThreads / 4)) {  // (uniform over the workgroup)
        const int r = r0 + (tid >> 2);
        double d = 0.0;
        if (r < n && lo < hi) {
            const float *a = p.a + (int64_t)r * p.stride;
            const double *b = p.b + (int64_t)r * p.nout;
            float am = -INFINITY;
            double b1 = -INFINITY, b2 = -INFINITY;
            int ai = lo, bi = lo;
            for (int c = lo; c < hi; ++c) {
                const float va = a[c];
                const double vb = b[c];
                d = fmax(d, fabs((double)va - vb));
                if (va > am) am = va, ai = c;
                if (vb > b1) b2 = b1, b1 = vb, bi = c;
                else if (vb > b2) b2 = vb;
            }
            if (ai != bi) {
                if (b1 - b2 > p.near_tie) ++t_label;
                else ++t_tie;
            }
            t_head = fmax(t_head, d);
        }
        d = fmax(d, __shfl_xor(d, 1, 64));
        d = fmax(d, __shfl_xor(d, 2, 64));
        if (h == 0 && r < n) {
            t_over += d > p.tol;
            verify_max_row64(t_max, t_row, d, (uint32_t)r);
        }
    }
    for (int off = 4; off < 64; off <<= 1) {
        t_head = fmax(t_head, __shfl_xor(t_head, off, 64));
        t_label += __shfl_xor(t_label, off, 64), t_tie += __shfl_xor(t_tie, off, 64), t_over += __shfl_xor(t_over, off, 64);
        const double om = __shfl_xor(t_max, off, 64);
        const uint32_t orow = __shfl_xor(t_row, off, 64);
        verify_max_row64(t_max, t_row, om, orow);
    }
    if (lane < 4) {
        VerifyRecord64 &w = wave_rec[tid >> 6];
        w.head_max[lane] = t_head, w.label[lane] = t_label, w.tie[lane] = t_tie;
        if (lane == 0) w.max_abs = t_max, w.worst_row = t_row, w.rows_over = t_over;
    }
    __syncthreads();
    if (tid == 0) {
        VerifyRecord64 o = wave_rec[0];
        for (int w = 1; w < kVerifyThreads / 64; ++w) {
            const VerifyRecord64 &v = wave_rec[w];
            verify_max_row64(o.max_abs, o.worst_row, v.max_abs, v.worst_row);
            o.rows_over += v.rows_over;
            for (int k = 0; k < 4; ++k) o.head_max[k] = fmax(o.head_max[k], v.head_max[k]), o.label[k] += v.label[k], o.tie[k] += v.tie[k];
        }
        p.part[blockIdx.x] = o;
    }
}

// one wave: the partials of n_parts workgroups -> the batch's record, and the double maximum at max64
template <int = 0>
__global__ __launch_bounds__(64) void rows_compare_f64_final_kernel(const VerifyRecord64 *part, int n_parts, const uint32_t *kept, int batch, VerifyRecord *out,
                                                                    double *max64) {
    const int lane = threadIdx.x;
    double mx = 0.0, hm[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t row = 0xffffffffu, over = 0, lab[4] = {0, 0, 0, 0}, tie[4] = {0, 0, 0, 0};
    for (int i = lane; i < n_parts; i += 64) {
        const VerifyRecord64 v = part[i];
        verify_max_row64(mx, row, v.max_abs, v.worst_row);
        over += v.rows_over;
#pragma unroll
        for (int k = 0; k < 4; ++k) hm[k] = fmax(hm[k], v.head_max[k]), lab[k] += v.label[k], tie[k] += v.tie[k];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(mx, off, 64);
        const uint32_t orow = __shfl_xor(row, off, 64);
        verify_max_row64(mx, row, om, orow);
        over += __shfl_xor(over, off, 64);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            hm[k] = fmax(hm[k], __shfl_xor(hm[k], off, 64)), lab[k] += __shfl_xor(lab[k], off, 64), tie[k] += __shfl_xor(tie[k], off, 64);
    }
    if (lane == 0) {
        VerifyRecord o;
        o.max_abs = (float)mx, o.worst_row = row == 0xffffffffu ? 0u : row, o.rows_over = over;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.head_max[k] = (float)hm[k], o.label[k] = lab[k], o.tie[k] = tie[k];
        o.n = kept ? min(*kept, (uint32_t)batch) : (uint32_t)batch;
        *out = o;
        *max64 = mx;
    }
}

// ---- layer records with the exact layers as the reference (c3_verify.h layer_compare_kernel says what is compared; here b is the fp64 tensor
// of c3_exact_fetch, in the checkpoint's units already: only a sheds its channel powers of two): |(double)a - b| in double, the record's
// floats the round-to-nearest floats of the double maxima.  A partial is as large as c3_verify.h's LayerRecord and lives in the same buffer
struct LayerRecord64 {
    double max_abs;
    float ref_max, test_max;
    uint32_t window, index;
    uint32_t pad[2];
};
static_assert(sizeof(LayerRecord64) == sizeof(LayerRecord), "the slot's buffer of layer partials holds either kind");
struct LayerCompareParams64 {
    const void *a;         // as LayerCompareParams
    const double *b;       // the exact layer of this pass [n][pw]
    const int *exp;
    const uint32_t *kept;
    LayerRecord64 *part;
    uint32_t pw8;
    int cshift, planes;
    uint32_t first, n, batch;
};
__device__ __forceinline__ double layer_abs64(double v) {  // |v|, +inf for anything not finite
    v = fabs(v);
    return v <= 1.7976931348623157e308 ? v : (double)INFINITY;
}
__device__ __forceinline__ void layer_max_pos64(double &m, uint32_t &w, uint32_t &i, double om, uint32_t ow, uint32_t oi) {
    if (om > m || (om == m && (ow < w || (ow == w && oi < i)))) m = om, w = ow, i = oi;
}

template <int = 0>
__global__ __launch_bounds__(kLayerThreads) void layer_compare_f64_kernel(LayerCompareParams64 p) {
    __shared__ LayerRecord64 wave_rec[kLayerThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t limit = p.kept ? min(*p.kept, p.batch) : p.batch;
    const uint32_t n = limit > p.first ? min(p.n, limit - p.first) : 0u;
    const uint32_t groups = n * p.pw8;
    const uint32_t cmask = (1u << p.cshift) - 1u;
    double t_max = 0.0, t_ref = 0.0;
    float t_test = 0.f;
    uint32_t t_win = 0xffffffffu, t_idx = 0xffffffffu;
    for (uint32_t g = blockIdx.x * kLayerThreads + tid; g < groups; g += gridDim.x * kLayerThreads) {  // ascending per thread
        const uint32_t w = g / p.pw8, i0 = (g - w * p.pw8) * 8u, c0 = (g & cmask) * 8u;
        float va[8];
        const double *b = p.b + (size_t)g * 8;
        if (p.planes) {
            const _Float16 *row = reinterpret_cast<const _Float16 *>(p.a) + ((size_t)(g >> p.cshift) << (p.cshift + 4)) + (c0 >> 6) * 128 + (c0 & 63);
            const layer_half8 hi = *reinterpret_cast<const layer_half8 *>(row), lo = *reinterpret_cast<const layer_half8 *>(row + 64);
#pragma unroll
            for (int k = 0; k < 8; ++k) va[k] = (float)hi[k] + (float)lo[k];
        } else {
            const float *a = reinterpret_cast<const float *>(p.a) + (size_t)g * 8;
            const float4 a0 = *reinterpret_cast<const float4 *>(a), a1 = *reinterpret_cast<const float4 *>(a + 4);
            va[0] = a0.x, va[1] = a0.y, va[2] = a0.z, va[3] = a0.w, va[4] = a1.x, va[5] = a1.y, va[6] = a1.z, va[7] = a1.w;
        }
        if (p.exp) {
#pragma unroll
            for (int k = 0; k < 8; ++k) va[k] = ldexpf(va[k], -p.exp[c0 + k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double vb = b[k], d = layer_abs64((double)va[k] - vb);
            if (d > t_max || t_win == 0xffffffffu) t_max = d, t_win = w, t_idx = i0 + k;
            t_ref = fmax(t_ref, layer_abs64(vb)), t_test = fmaxf(t_test, layer_abs(va[k]));
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(t_max, off, 64);
        const uint32_t ow = __shfl_xor(t_win, off, 64), oi = __shfl_xor(t_idx, off, 64);
        layer_max_pos64(t_max, t_win, t_idx, om, ow, oi);
        t_ref = fmax(t_ref, __shfl_xor(t_ref, off, 64)), t_test = fmaxf(t_test, __shfl_xor(t_test, off, 64));
    }
    if (lane == 0) {
        LayerRecord64 &r = wave_rec[tid >> 6];
        r.max_abs = t_max, r.ref_max = (float)t_ref, r.test_max = t_test, r.window = t_win, r.index = t_idx;
    }
    __syncthreads();
    if (tid == 0) {
        LayerRecord64 o = wave_rec[0];
        for (int w = 1; w < kLayerThreads / 64; ++w) {
            const LayerRecord64 &v = wave_rec[w];
            layer_max_pos64(o.max_abs, o.window, o.index, v.max_abs, v.window, v.index);
            o.ref_max = fmaxf(o.ref_max, v.ref_max), o.test_max = fmaxf(o.test_max, v.test_max);
        }
        if (o.window != 0xffffffffu) o.window += p.first;  // the window's number in the batch
        o.pad[0] = o.pad[1] = 0;
        p.part[blockIdx.x] = o;
    }
}

// one wave per layer: its fp64 partials (LayerFinalParams::part read as LayerRecord64) -> its record of the batch
template <int = 0>
__global__ __launch_bounds__(64) void layer_compare_f64_final_kernel(LayerFinalParams p) {
    const int lane = threadIdx.x, k = blockIdx.x, np = p.n_parts[k];
    const LayerRecord64 *part = reinterpret_cast<const LayerRecord64 *>(p.part) + p.part_at[k];
    double mx = 0.0;
    float ref = 0.f, test = 0.f;
    uint32_t win = 0xffffffffu, idx = 0xffffffffu;
    for (int i = lane; i < np; i += 64) {
        const LayerRecord64 v = part[i];
        layer_max_pos64(mx, win, idx, v.max_abs, v.window, v.index);
        ref = fmaxf(ref, v.ref_max), test = fmaxf(test, v.test_max);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(mx, off, 64);
        const uint32_t ow = __shfl_xor(win, off, 64), oi = __shfl_xor(idx, off, 64);
        layer_max_pos64(mx, win, idx, om, ow, oi);
        ref = fmaxf(ref, __shfl_xor(ref, off, 64)), test = fmaxf(test, __shfl_xor(test, off, 64));
    }
    if (lane == 0) {
        LayerRecord o;
        o.max_abs = (float)mx, o.ref_max = ref, o.test_max = test;
        o.window = win == 0xffffffffu ? 0u : win, o.index = win == 0xffffffffu ? 0u : idx;
        o.windows = np == 0 ? 0u : p.kept ? min(*p.kept, (uint32_t)p.batch) : (uint32_t)p.batch;
        o.compared = np != 0, o.pad = 0;
        p.out[k] = o;
    }
}

// ---- C3_VERIFY_REPLACE: one thread per row decides by the rule of the compare kernel of its reference (R = float: rows_compare_kernel's
// fp32 arithmetic; R = double: the one above) -- a row over tol, or with an arg-max difference outside near-ties in any head -- and
// overwrites such a row of a with the reference's float32 row; every other row is not touched.  The count is an integer sum: it does not
// depend on scheduling
template <class R>
struct ReplaceParams {
    float *a;              // the rows under test [batch][stride], repaired in place
    const R *b;            // the reference's rows [batch][bstride]
    const float *bf;       // ... as float32 [batch][stride]: what a replaced row becomes (R = float: b itself)
    const uint32_t *kept;  // as CompareParams
    uint32_t *count;       // rows replaced (zeroed in front of the launch)
    int stride, bstride, nout, batch;
    R tol, near_tie;
};
template <class R>
__global__ __launch_bounds__(256) void rows_replace_kernel(ReplaceParams<R> p) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int n = p.kept ? (int)min(*p.kept, (uint32_t)p.batch) : p.batch;
    if (r >= n) return;
    float *a = p.a + (int64_t)r * p.stride;
    const R *b = p.b + (int64_t)r * p.bstride;
    bool bad = false;
    R row_d = (R)0;
    for (int h = 0; h < 4; ++h) {
        const int lo = h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57;
        const int hi = min(h == 0 ? 21 : h == 1 ? 24 : h == 2 ? 57 : 90, p.nout);
        if (lo >= hi) continue;
        float am = -INFINITY;
        R b1 = -INFINITY, b2 = -INFINITY, d = (R)0;
        int ai = lo, bi = lo;
        for (int c = lo; c < hi; ++c) {
            const float va = a[c];
            const R vb = b[c];
            if constexpr (sizeof(R) == 8) d = fmax(d, fabs((double)va - vb));
            else d = fmaxf(d, fabsf(va - vb));
            if (va > am) am = va, ai = c;
            if (vb > b1) b2 = b1, b1 = vb, bi = c;
            else if (vb > b2) b2 = vb;
        }
        bad |= ai != bi && b1 - b2 > p.near_tie;
        if constexpr (sizeof(R) == 8) row_d = fmax(row_d, d);
        else row_d = fmaxf(row_d, d);
    }
    bad |= row_d > p.tol;
    if (!bad) return;
    const float *src = p.bf + (int64_t)r * p.stride;
    for (int c = 0; c < p.nout; ++c) a[c] = src[c];
    atomicAdd(p.count, 1u);
}

}  // namespace c3

// ------------------------------------------------------------------------------------------ host
template <class L, int EPI>
static int exact_gemm(hipStream_t s, const typename L::Params &lp, const double *w, const double *bias, const double *res, double *out,
                      int64_t M, int N, int K, int64_t ldc) {
    if (M <= 0) return 0;
    if (M > ((int64_t)1 << 30)) return fail("c3_predict_exact: pass too large (%lld rows)", (long long)M);
    ExGemm g{w, bias, res, out, (int)M, N, K, ldc};
    const dim3 grid((unsigned)((M + kExBM - 1) / kExBM), (unsigned)((N + kExBN - 1) / kExBN));
    hipLaunchKernelGGL((exact_gemm_kernel<L, EPI>), grid, dim3(256), 0, s, lp, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int64_t exact_chunk(const c3_model *m) {
    int64_t n = m->kind == C3_KIND_PILEUP ? 1024 : 256;
    if (const char *e = getenv("C3HIP_EXACT_CHUNK")) n = atoll(e);
    return std::min<int64_t>(std::max<int64_t>(n, 1), 4096);
}

static int exact_ws_alloc(ExactState &E, void **p, size_t bytes) {
    HIP_TRY(hipMalloc(p, std::max<size_t>(bytes, 256)));
    E.ws.push_back(*p);
    return 0;
}

// the workspace of a pass of n windows
static int exact_ensure_workspace(c3_model *m, int64_t n, int item) {
    ExactState &E = m->exact;
    const size_t xbytes = (size_t)c3_model_window_bytes(m, item == 4 ? C3_DTYPE_I32 : C3_DTYPE_I8);
    if (n <= E.cap && xbytes <= E.x_window_bytes) return 0;
    n = std::max(n, E.cap);
    HIP_TRY(hipDeviceSynchronize());
    exact_free_workspace(m);
    auto D = [&](double **p, size_t elems) { return exact_ws_alloc(E, (void **)p, elems * (size_t)n * sizeof(double)); };
    TRY(exact_ws_alloc(E, &E.x, xbytes * (size_t)n));
    if (m->kind == C3_KIND_FULL_ALIGNMENT) {
        int hh[10], ww[10];
        fa_geometry(m, hh, ww);
        for (int l = 0; l < 9; ++l) TRY(D(&E.act[l], (size_t)hh[l + 1] * ww[l + 1] * kConvCout[l]));
        TRY(D(&E.spp, (size_t)m->K4));
    } else {
        const size_t T = (size_t)m->positions;
        TRY(D(&E.gx1, T * 1024));
        TRY(D(&E.h1, T * 256));
        TRY(D(&E.gx2, T * 1280));
        TRY(D(&E.h2, T * 320));
    }
    TRY(D(&E.l4, (size_t)m->FC));
    TRY(D(&E.l5, (size_t)m->nb * 128));
    TRY(D(&E.logit, (size_t)m->nout));
    TRY(D(&E.y, (size_t)m->nout));
    E.cap = n, E.x_window_bytes = xbytes;
    return 0;
}

// one pass: n windows at x (device) -> E.y, every layer output left in the workspace
static int exact_pass(c3_model *m, hipStream_t s, const void *x, int x_dtype, int64_t n) {
    ExactState &E = m->exact;
    typedef ExDense<double> DD;
    if (m->kind == C3_KIND_PILEUP) {
        const int T = m->positions;
        const int64_t M = n * T;
        // clair3/model.py:131-133: x.float(), LSTM1, LSTM2 (both bidirectional); the input projections of all steps as one contraction each
        if (x_dtype == C3_DTYPE_I32)
            TRY((exact_gemm<ExDense<int32_t>, kExBias>(s, {(const int32_t *)x, m->C}, E.wih[0], E.pb[0], nullptr, E.gx1, M, 1024, m->C, 1024)));
        else
            TRY((exact_gemm<ExDense<int8_t>, kExBias>(s, {(const int8_t *)x, m->C}, E.wih[0], E.pb[0], nullptr, E.gx1, M, 1024, m->C, 1024)));
        const dim3 grid((unsigned)((n + 15) / 16), 2);
        hipLaunchKernelGGL(exact_lstm_kernel<128>, grid, dim3(128 / 16 * 64), 0, s, E.gx1, E.whh[0], E.h1, (int)n, T);
        HIP_TRY(hipGetLastError());
        TRY((exact_gemm<DD, kExBias>(s, {E.h1, 256}, E.wih[1], E.pb[1], nullptr, E.gx2, M, 1280, 256, 1280)));
        hipLaunchKernelGGL(exact_lstm_kernel<160>, grid, dim3(160 / 16 * 64), 0, s, E.gx2, E.whh[1], E.h2, (int)n, T);
        HIP_TRY(hipGetLastError());
        // model.py:135-136: flatten, L4, SELU
        TRY((exact_gemm<DD, kExBiasSelu>(s, {E.h2, m->K4}, E.l4w, E.l4b, nullptr, E.l4, n, m->FC, m->K4, m->FC)));
    } else {
        int hh[10], ww[10];
        fa_geometry(m, hh, ww);
        int cin = m->C;
        for (int l = 0; l < 9; ++l) {  // model.py:378-392: conv + BatchNorm + ReLU, the identity of a residual block added before its last ReLU
            const int Cout = kConvCout[l];
            const int64_t M = n * hh[l + 1] * ww[l + 1];
            const double *res = l % 3 == 2 ? E.act[l - 2] : nullptr;
            if (l == 0)
                TRY((exact_gemm<ExConv<int8_t, true>, kExBiasResRelu>(s, {(const int8_t *)x, hh[0], ww[0], cin, hh[1], ww[1], kConvStride[0]},
                                                                     E.cw[0], E.cb[0], res, E.act[0], M, Cout, 9 * cin, Cout)));
            else
                TRY((exact_gemm<ExConv<double, false>, kExBiasResRelu>(s, {E.act[l - 1], hh[l], ww[l], cin, hh[l + 1], ww[l + 1], kConvStride[l]},
                                                                      E.cw[l], E.cb[l], res, E.act[l], M, Cout, 9 * cin, Cout)));
            cin = Cout;
        }
        SppParams sp;
        TRY(spp_bins(m, hh[9], ww[9], sp));
        sp.in = nullptr, sp.out = nullptr, sp.B = (int)n;
        const int64_t total = n * sp.nbins * 256;
        hipLaunchKernelGGL(exact_spp_kernel<>, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 65535)), dim3(256), 0, s, sp, E.act[8], E.spp);
        HIP_TRY(hipGetLastError());
        TRY((exact_gemm<DD, kExBiasSelu>(s, {E.spp, m->K4}, E.l4w, E.l4b, nullptr, E.l4, n, m->FC, m->K4, m->FC)));
    }
    // the FC tail of both networks, model.py:139-159: L5_k + SELU, the heads, softmax(selu(.))
    const int n5 = m->nb * 128;
    TRY((exact_gemm<DD, kExBiasSelu>(s, {E.l4, m->FC}, E.w5, E.b5, nullptr, E.l5, n, n5, m->FC, n5)));
    for (int br = 0, off = 0; br < m->nb; off += kHeadN[br], ++br)
        TRY((exact_gemm<DD, kExBias>(s, {E.l5 + br * 128, n5}, E.wh + (size_t)off * 128, E.bh + off, nullptr, E.logit + off, n, kHeadN[br], 128, m->nout)));
    hipLaunchKernelGGL(exact_softmax_kernel<>, dim3((unsigned)((n * m->nb + 255) / 256)), dim3(256), 0, s, E.logit, E.y, n, m->nb, m->nout);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ on the ring (c3_hostring.h launch_batch, shadow_pass)
// the active lane's buffers of gathered / rescaled (c3_rescale.h) and expanded (c3_expand.h) windows, for a pass of n windows: the product
// pass sizes them by its workspace (c3_model.h ensure_rescale_buf, ensure_expand_buf), which an exact-answer handle may never allocate
static int exact_ensure_lane_windows(c3_model *m, int64_t n, bool gathered, bool expanded) {
    Lane &L = lane(m);
    if (gathered && L.xr_cap < n) {
        HIP_TRY(hipDeviceSynchronize());  // (a batch in flight in this lane may still read the smaller one)
        if (L.xr) (void)hipFree(L.xr);
        L.xr = nullptr, L.xr_cap = 0;
        HIP_TRY(hipMalloc((void **)&L.xr, std::max<size_t>((size_t)n * m->positions * m->C * sizeof(int32_t), 256)));
        L.xr_cap = n;
    }
    if (expanded && L.xe_cap < n) {
        HIP_TRY(hipDeviceSynchronize());
        if (L.xe) (void)hipFree(L.xe);
        L.xe = nullptr, L.xe_cap = 0;
        HIP_TRY(hipMalloc((void **)&L.xe, std::max<size_t>((size_t)n * m->depth * m->positions * m->C, 256)));
        L.xe_cap = n;
    }
    return 0;
}

// layer records against the exact layers (c3_model_set_verify_layers under C3_VERIFY_REF_EXACT): behind a pass of n windows from window
// `first` of the batch, every layer the product pass kept in the slot (c3_forward.h layer_tap, pass 1) against the exact layer of this pass.
// The partials share the slot's buffer with the fp32 reference's: blocks_cap per launch keeps all passes of a batch inside a layer's share
static int exact_layers_compare(c3_model *m, hipStream_t s, HostSlot &sl, int64_t first, int64_t n, int blocks_cap) {
    ExactState &E = m->exact;
    if (sl.layer_dropped) return 0;
    int ids[kLayerMaxLayers];
    const int nl = verify_layer_ids(m, ids);
    for (int k = 0; k < nl; ++k) {
        const int id = ids[k];
        if (!(sl.layer_kept >> id & 1u)) continue;
        const int64_t pw = tap_window_floats(m, id);
        if (pw % 8) return fail("internal: %s has %lld values per window, the compare kernel takes 8 at a time", kTapName[id], (long long)pw);
        const int blocks = (int)std::min<int64_t>(blocks_cap, std::max<int64_t>(1, (n * (pw / 8) + kLayerThreads - 1) / kLayerThreads));
        if (sl.layer_parts[id] + blocks > sl.layer_part_stride) return fail("internal: layer partials of %s", kTapName[id]);
        LayerCompareParams64 cp;
        cp.a = sl.layer_buf[id] + first * pw;
        cp.b = id <= 8 ? E.act[id] : id == kTapSpp ? E.spp : id == kTapL4 ? E.l4 : id == kTapLstm1 ? E.h1 : id == kTapGx2 ? E.gx2 : E.h2;
        cp.exp = nullptr, cp.cshift = 0, cp.kept = m->layer_kept_count;
        cp.part = reinterpret_cast<LayerRecord64 *>(sl.layer_part) + (size_t)id * sl.layer_part_stride + sl.layer_parts[id];
        cp.pw8 = (uint32_t)(pw / 8), cp.planes = (sl.layer_planes >> id & 1u) != 0;
        cp.first = (uint32_t)first, cp.n = (uint32_t)n, cp.batch = (uint32_t)m->layer_batch;
        int C = cp.planes ? (m->kind == C3_KIND_PILEUP ? 256 : kConvCout[id]) : 8;
        if (m->kind == C3_KIND_FULL_ALIGNMENT && id <= kTapSpp && !m->act_exp[std::min(id, 8)].empty())
            cp.exp = m->layer_exp + std::min(id, 8) * 256, C = (int)m->act_exp[std::min(id, 8)].size();
        while ((8 << cp.cshift) < C) ++cp.cshift;
        if ((8 << cp.cshift) != C || pw % C) return fail("internal: %s has %d channels", kTapName[id], C);
        hipLaunchKernelGGL(layer_compare_f64_kernel<>, dim3((unsigned)blocks), dim3(kLayerThreads), 0, s, cp);
        HIP_TRY(hipGetLastError());
        sl.layer_parts[id] += blocks;
    }
    return 0;
}

// The batch staged in slot sl through the exact form, on stream s (the active lane's): passes of C3HIP_EXACT_CHUNK windows, each read from
// where the product forms would read it -- the staged image; with depths, or for a region / candidate batch (whose plan always carries
// depths: c3_hostring.h predict_submit), what rescale_windows_kernel wrote into the lane's buffer; with a rows table, Lane::xe -- and rounded
// to float32 into y (row stride m->row, decoder columns filled in), the doubles of the whole batch to keep64 when given.  The workspace is
// the handle's: the event puts this batch's passes behind those of the batch before it, whatever lane that ran in
static int exact_ring_pass(c3_model *m, hipStream_t s, HostSlot &sl, const StagedBatch &p, int x_dtype, int64_t batch, float *y, double *keep64,
                           bool layers) {
    ExactState &E = m->exact;
    if (!E.loaded) return fail("the exact form was not enabled at the last load: c3_model_set_exact(m, 1), then c3_model_load");
    if (batch <= 0) return 0;
    const int32_t *starts = sl.dev<const int32_t>(p.starts), *depth = sl.dev<const int32_t>(p.depth);
    const ExpandEntry *rows = sl.dev<const ExpandEntry>(p.rows_tab);
    if ((starts || depth) && (m->kind != C3_KIND_PILEUP || x_dtype != C3_DTYPE_I32)) return fail("internal: the exact form gathers int32 pileup counts");
    if (starts && !depth) return fail("internal: a region batch for the exact form was staged without depths");
    if (rows && (m->kind != C3_KIND_FULL_ALIGNMENT || x_dtype != C3_DTYPE_I8)) return fail("internal: rows need int8 full-alignment windows");
    if (x_dtype != C3_DTYPE_I8 && !(x_dtype == C3_DTYPE_I32 && m->kind == C3_KIND_PILEUP))
        return fail("%s windows must be %s", m->kind == C3_KIND_PILEUP ? "pileup" : "full-alignment", m->kind == C3_KIND_PILEUP ? "int8 or int32" : "int8");
    const int64_t chunk = exact_chunk(m), cap = std::min(batch, chunk);
    TRY(exact_ensure_workspace(m, cap, x_dtype == C3_DTYPE_I32 ? 4 : 1));
    TRY(exact_ensure_lane_windows(m, cap, depth != nullptr, rows != nullptr));
    if (!E.ring_ev) HIP_TRY(hipEventCreateWithFlags(&E.ring_ev, hipEventDisableTiming));
    if (E.ring_recorded) HIP_TRY(hipStreamWaitEvent(s, E.ring_ev, 0));
    Lane &L = lane(m);
    const int64_t wbytes = c3_model_window_bytes(m, x_dtype);
    for (int64_t off = 0; off < batch; off += chunk) {
        const int64_t n = std::min(chunk, batch - off);
        ProfScope ps(m, s, m->kind == C3_KIND_PILEUP ? "p.exact" : "fa.exact", 0.0, (double)n * (double)wbytes);
        const void *x = (const char *)sl.dev_x + off * wbytes;
        if (rows) {
            ExpandParams ep{(const int8_t *)sl.dev_x, rows + off, L.xe, (int)n, m->positions * m->C, (int)wbytes};
            if (ep.row_bytes % 8 == 0) hipLaunchKernelGGL(expand_rows_kernel<8>, dim3((unsigned)n), dim3(kExpandThreads), 0, s, ep);
            else hipLaunchKernelGGL(expand_rows_kernel<1>, dim3((unsigned)n), dim3(kExpandThreads), 0, s, ep);
            HIP_TRY(hipGetLastError());
            x = L.xe;
        } else if (depth) {
            const int TC = m->positions * m->C;
            RescaleParams rp{(const int32_t *)(starts ? sl.dev_x : x), starts ? starts + off : nullptr, depth + off, L.xr, (int)n, TC, m->C, m->max_depth};
            const dim3 grid((unsigned)((n + kRescaleWindows - 1) / kRescaleWindows));
            if (m->C % 2 == 0) hipLaunchKernelGGL(rescale_windows_kernel<2>, grid, dim3(kRescaleThreads), 0, s, rp);
            else hipLaunchKernelGGL(rescale_windows_kernel<1>, grid, dim3(kRescaleThreads), 0, s, rp);
            HIP_TRY(hipGetLastError());
            x = L.xr;
        }
        TRY(exact_pass(m, s, x, x_dtype, n));
        hipLaunchKernelGGL(exact_rows_to_f32_kernel<>, dim3((unsigned)((n * m->nout + 255) / 256)), dim3(256), 0, s, (const double *)E.y, y + off * m->row,
                           keep64 ? keep64 + off * m->nout : (double *)nullptr, n, m->nout, m->row);
        HIP_TRY(hipGetLastError());
        if (layers) {  // (the exact layers exist one pass at a time: compared here, behind the pass that wrote them)
            const int64_t passes = (batch + chunk - 1) / chunk;
            if (passes > sl.layer_part_stride) return fail("internal: %lld exact passes for %d layer partials", (long long)passes, sl.layer_part_stride);
            TRY(exact_layers_compare(m, s, sl, off, n, (int)std::min<int64_t>(kLayerMaxBlocks, sl.layer_part_stride / passes)));
        }
        E.last_n = n;
    }
    HIP_TRY(hipEventRecord(E.ring_ev, s));
    E.ring_recorded = true;
    if (m->row > m->nout) {  // decoder columns behind the probabilities of every row (c3_decode.h), as run_tail fills them
        DecodeParams dp{y, m->row, nullptr, nullptr, nullptr, nullptr, y + m->nout, (int)batch, m->nout == 90 ? 1 : 0};
        hipLaunchKernelGGL(outcome_maxima_kernel<true>, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, s, dp);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// Refine mode's second pass (c3_refine.h; c3_hostring.h refine_account calls it from c3_predict_wait): the n_sel selected windows of the batch
// that came home in slot sl, in the batch's lane.  Per pass of C3HIP_EXACT_CHUNK windows: gathered from the staged image into the exact
// form's own window buffer (ExactState::x, the handle's: grown on demand, freed with it), exact_pass, the rows rounded to float32 into the
// handle's compact row buffer; then the decoder columns of those rows, the scatter into the batch's rows -- in the slot, or in the caller's
// device buffer --, the repaired rows and the record on their way to the pinned buffer, one synchronize.  Ordered behind the passes of other
// lanes by ExactState::ring_ev as exact_ring_pass is
static int refine_pass(c3_model *m, HostSlot &sl, int64_t n_sel) {
    ExactState &E = m->exact;
    const StagedBatch &p = sl.plan;
    if (!E.loaded) return fail("refine mode: the exact form was not enabled at the last load: c3_model_set_exact(m, 1), then c3_model_load");
    TRY(use_lane(m, sl.lane));
    hipStream_t s = lane(m).stream;
    char *section = (char *)sl.dev_y + p.refine.off;
    const int32_t *index = (const int32_t *)(section + kRefineRecordBytes);
    const int64_t chunk = exact_chunk(m), wbytes = c3_model_window_bytes(m, sl.x_dtype);
    TRY(exact_ensure_workspace(m, std::min(n_sel, chunk), sl.x_dtype == C3_DTYPE_I32 ? 4 : 1));
    const size_t row_bytes = (size_t)n_sel * m->row * sizeof(float);
    if (row_bytes > m->refine_rows_bytes) {  // (every earlier second pass ended with a synchronize: nothing reads the smaller one)
        if (m->refine_rows) (void)hipFree(m->refine_rows);
        m->refine_rows = nullptr, m->refine_rows_bytes = 0;
        HIP_TRY(hipMalloc((void **)&m->refine_rows, row_bytes));
        m->refine_rows_bytes = row_bytes;
    }
    if (!E.ring_ev) HIP_TRY(hipEventCreateWithFlags(&E.ring_ev, hipEventDisableTiming));
    if (E.ring_recorded) HIP_TRY(hipStreamWaitEvent(s, E.ring_ev, 0));
    for (int64_t off = 0; off < n_sel; off += chunk) {
        const int64_t n = std::min(chunk, n_sel - off);
        if (wbytes % 8 == 0) hipLaunchKernelGGL(refine_gather_kernel<8>, dim3((unsigned)n), dim3(256), 0, s, (const char *)sl.dev_x, index + off, (char *)E.x, wbytes);
        else hipLaunchKernelGGL(refine_gather_kernel<1>, dim3((unsigned)n), dim3(256), 0, s, (const char *)sl.dev_x, index + off, (char *)E.x, wbytes);
        HIP_TRY(hipGetLastError());
        TRY(exact_pass(m, s, E.x, sl.x_dtype, n));
        hipLaunchKernelGGL(exact_rows_to_f32_kernel<>, dim3((unsigned)((n * m->nout + 255) / 256)), dim3(256), 0, s, (const double *)E.y,
                           m->refine_rows + off * m->row, (double *)nullptr, n, m->nout, m->row);
        HIP_TRY(hipGetLastError());
        E.last_n = n;
    }
    HIP_TRY(hipEventRecord(E.ring_ev, s));
    E.ring_recorded = true;
    if (m->row > m->nout) {  // decoder columns of the refined rows, from their refined probabilities
        DecodeParams dp{m->refine_rows, m->row, nullptr, nullptr, nullptr, nullptr, m->refine_rows + m->nout, (int)n_sel, m->nout == 90 ? 1 : 0};
        hipLaunchKernelGGL(outcome_maxima_kernel<true>, dim3((unsigned)((n_sel + 3) / 4)), dim3(256), 0, s, dp);
        HIP_TRY(hipGetLastError());
    }
    RefineScatterParams sp;
    sp.refined = m->refine_rows, sp.index = index, sp.rows = sl.y_dev_out ? sl.y_dev_out : sl.dev_y, sp.rec = (RefineRecord *)section;
    sp.stride = m->row, sp.nout = m->nout, sp.n = (int)n_sel;
    hipLaunchKernelGGL(refine_scatter_kernel, dim3(refine_blocks(n_sel)), dim3(kRefineThreads), 0, s, sp);
    HIP_TRY(hipGetLastError());
    // rows that came to this host: the batch's rows and its record again (one transfer: the sections lie behind each other); rows that stay on
    // the device: the record
    if (sl.y_dev_out) HIP_TRY(hipMemcpyAsync((char *)sl.pin_y + p.refine.off, section, kRefineRecordBytes, hipMemcpyDeviceToHost, s));
    else HIP_TRY(hipMemcpyAsync(sl.pin_y, sl.dev_y, p.refine.off + kRefineRecordBytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// C3_VERIFY_REPLACE behind the comparison (either reference): the rows under test are repaired where they are, in front of their copy-out;
// the count lands in the verify record's section.  ref64: the exact rows (nullptr: the reference is the fp32 rows at the front of sl.shadow)
static int verify_replace_launch(c3_model *m, hipStream_t s, HostSlot &sl, const RingInput &in, const StagedBatch &p, const double *ref64) {
    float *a = in.y_dev ? in.y_dev : sl.dev_y;
    const uint32_t *kept = in.kind == InKind::Candidates ? (const uint32_t *)((const char *)sl.dev_y + p.kept.off) : nullptr;
    uint32_t *count = (uint32_t *)((char *)sl.dev_y + p.verify.off + kVerifyReplacedAt);
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
    const dim3 grid((unsigned)((in.batch + 255) / 256));
    if (ref64) {
        ReplaceParams<double> rp{a, ref64, sl.shadow, kept, count, m->row, m->nout, m->nout, (int)in.batch, (double)m->verify_tol, (double)m->verify_near_tie};
        hipLaunchKernelGGL(rows_replace_kernel<double>, grid, dim3(256), 0, s, rp);
    } else {
        ReplaceParams<float> rp{a, sl.shadow, sl.shadow, kept, count, m->row, m->row, m->nout, (int)in.batch, m->verify_tol, m->verify_near_tie};
        hipLaunchKernelGGL(rows_replace_kernel<float>, grid, dim3(256), 0, s, rp);
    }
    HIP_TRY(hipGetLastError());
    if (m->row > m->nout) {  // the decoder columns of the batch, from the rows as they now are (an untouched row gives the columns it had)
        DecodeParams dp{a, m->row, nullptr, nullptr, nullptr, nullptr, a + m->nout, (int)in.batch, m->nout == 90 ? 1 : 0};
        hipLaunchKernelGGL(outcome_maxima_kernel<true>, dim3((unsigned)((in.batch + 3) / 4)), dim3(256), 0, s, dp);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// verify mode's second pass with the exact form as the reference (c3_hostring.h shadow_pass is the fp32 one): the exact pass from the same
// staged input, its float32 rows at the front of the slot's shadow buffer, its doubles behind them; the fp64 compare kernels; the record
// lands where shadow_pass puts it, the double maximum behind it
static int exact_shadow_pass(c3_model *m, HostSlot &sl, const RingInput &in, const StagedBatch &p) {
    hipStream_t s = lane(m).stream;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t rows64 = al(p.y.bytes), part = rows64 + al((size_t)in.batch * m->nout * sizeof(double));
    const size_t bytes = part + (size_t)kVerifyMaxBlocks * sizeof(VerifyRecord64);
    if (bytes > sl.shadow_bytes) {  // (the slot is free: nothing reads the buffer)
        if (sl.shadow) (void)hipFree(sl.shadow);
        sl.shadow = nullptr, sl.shadow_bytes = 0;
        HIP_TRY(hipMalloc((void **)&sl.shadow, bytes));
        sl.shadow_bytes = bytes;
    }
    sl.shadow_rows64 = rows64, sl.shadow_part = part;
    double *y64 = (double *)((char *)sl.shadow + rows64);
    TRY(exact_ring_pass(m, s, sl, p, in.x_dtype, in.batch, sl.shadow, y64, p.layers.bytes != 0));
    if (p.layers.bytes) {  // one wave per layer: the partials of its launches -> its record (as c3_hostring.h shadow_pass, the partials fp64)
        LayerFinalParams fp;
        int ids[kLayerMaxLayers];
        const int nl = verify_layer_ids(m, ids);
        fp.part = sl.layer_part, fp.kept = m->layer_kept_count, fp.out = (LayerRecord *)((char *)sl.dev_y + p.layers.off);
        fp.batch = (int)in.batch;
        for (int k = 0; k < kLayerMaxLayers; ++k) fp.part_at[k] = fp.n_parts[k] = 0;
        for (int k = 0; k < nl; ++k) fp.part_at[k] = ids[k] * sl.layer_part_stride, fp.n_parts[k] = sl.layer_parts[ids[k]];
        hipLaunchKernelGGL(layer_compare_f64_final_kernel<>, dim3((unsigned)nl), dim3(64), 0, s, fp);
        HIP_TRY(hipGetLastError());
    }
    CompareParams64 cp;
    cp.a = in.y_dev ? in.y_dev : sl.dev_y, cp.b = y64;
    cp.kept = in.kind == InKind::Candidates ? (const uint32_t *)((const char *)sl.dev_y + p.kept.off) : nullptr;
    cp.part = (VerifyRecord64 *)((char *)sl.shadow + part);
    cp.stride = m->row, cp.nout = m->nout, cp.batch = (int)in.batch, cp.tol = (double)m->verify_tol, cp.near_tie = (double)m->verify_near_tie;
    const int blocks = (int)std::min<int64_t>(kVerifyMaxBlocks, (in.batch + kVerifyThreads / 4 - 1) / (kVerifyThreads / 4));
    hipLaunchKernelGGL(rows_compare_f64_kernel<>, dim3((unsigned)blocks), dim3(kVerifyThreads), 0, s, cp);
    HIP_TRY(hipGetLastError());
    char *rec = (char *)sl.dev_y + p.verify.off;
    hipLaunchKernelGGL(rows_compare_f64_final_kernel<>, dim3(1), dim3(64), 0, s, (const VerifyRecord64 *)cp.part, blocks, cp.kept, (int)in.batch, (VerifyRecord *)rec,
                       (double *)(rec + kVerifyMax64At));
    HIP_TRY(hipGetLastError());
    if (m->verify_policy == C3_VERIFY_REPLACE) TRY(verify_replace_launch(m, s, sl, in, p, y64));
    return 0;
}

extern "C" {

int c3_model_set_exact(c3_model *m, int enable) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (!enable && m->answer_exact) return fail("c3_model_set_exact: the handle answers from the exact form: c3_model_set_answer(m, C3_ANSWER_PRODUCT) first");
    if (!enable && m->verify_ref == C3_VERIFY_REF_EXACT)
        return fail("c3_model_set_exact: verify mode's reference is the exact form: c3_model_set_verify_reference(m, C3_VERIFY_REF_FP32) first");
    if (!enable && m->refine_on) return fail("c3_model_set_exact: refine mode answers near-ties from the exact form: c3_model_set_refine(m, 0, 0) first");
    m->exact.want = enable != 0;
    return 0;
}

int c3_predict_exact(c3_model *m, const void *x_host, int x_dtype, int64_t batch, double *y_host) {
    if (!m) return fail("c3_predict_exact: null model");
    if (batch < 0) return fail("c3_predict_exact: negative batch");
    if (!m->loaded) return fail("c3_predict_exact: no weights loaded");
    if (!m->exact.loaded) return fail("c3_predict_exact: the exact form was not enabled at the last load: c3_model_set_exact(m, 1), then c3_model_load");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("c3_predict_exact: a prediction is in flight: call c3_predict_wait first");
    if (x_dtype != C3_DTYPE_I8 && !(x_dtype == C3_DTYPE_I32 && m->kind == C3_KIND_PILEUP))
        return fail("c3_predict_exact: %s windows must be %s", m->kind == C3_KIND_PILEUP ? "pileup" : "full-alignment",
                    m->kind == C3_KIND_PILEUP ? "int8 or int32" : "int8");
    if (batch == 0) return 0;
    if (!x_host || !y_host) return fail("c3_predict_exact: null buffer");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());  // (the device-resident entries may still be running on a caller's stream)
    const int64_t chunk = exact_chunk(m);
    TRY(exact_ensure_workspace(m, std::min(batch, chunk), x_dtype == C3_DTYPE_I32 ? 4 : 1));
    ExactState &E = m->exact;
    hipStream_t s = m->lanes[0].stream;  // the first lane's stream, fully synchronised before and behind: nothing of the handle is in flight
    const size_t wbytes = (size_t)c3_model_window_bytes(m, x_dtype);
    E.last_n = 0;
    for (int64_t off = 0; off < batch; off += chunk) {
        const int64_t n = std::min(chunk, batch - off);
        TRY(h2d_staged(E.x, (const char *)x_host + (size_t)off * wbytes, (size_t)n * wbytes, s));
        TRY(exact_pass(m, s, E.x, x_dtype, n));
        TRY(d2h_staged(y_host + off * m->nout, E.y, (size_t)n * m->nout * sizeof(double), s));
        HIP_TRY(hipStreamSynchronize(s));
        E.last_n = n;
    }
    return 0;
}

int c3_model_set_answer(c3_model *m, int form) {
    if (!m) return fail("c3_model_set_answer: null model");
    if (form != C3_ANSWER_PRODUCT && form != C3_ANSWER_EXACT) return fail("c3_model_set_answer: form must be C3_ANSWER_PRODUCT or C3_ANSWER_EXACT, got %d", form);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (form == C3_ANSWER_EXACT && !m->exact.loaded)
        return fail("c3_model_set_answer: the exact form was not enabled at the last load: c3_model_set_exact(m, 1), then c3_model_load");
    m->answer_exact = form == C3_ANSWER_EXACT;
    return 0;
}

int c3_model_set_verify_reference(c3_model *m, int ref) {
    if (!m) return fail("c3_model_set_verify_reference: null model");
    if (ref != C3_VERIFY_REF_FP32 && ref != C3_VERIFY_REF_EXACT)
        return fail("c3_model_set_verify_reference: ref must be C3_VERIFY_REF_FP32 or C3_VERIFY_REF_EXACT, got %d", ref);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (ref == C3_VERIFY_REF_EXACT && !m->exact.loaded)
        return fail("c3_model_set_verify_reference: the exact form was not enabled at the last load: c3_model_set_exact(m, 1), then c3_model_load");
    m->verify_ref = ref;
    return 0;
}

int c3_model_verify_extra(c3_model *m, c3_verify_extra *out) {
    if (!m || !out) return fail("c3_model_verify_extra: null argument");
    *out = m->vextra;
    out->reference = m->verify_ref, out->reserved = 0;
    return 0;
}

int c3_exact_fetch(c3_model *m, const char *name, int64_t first, int64_t windows, double *host_out, int64_t n_doubles) {
    if (!m) return fail("c3_exact_fetch: null model");
    if (!name || (!host_out && n_doubles > 0)) return fail("c3_exact_fetch: null argument");
    ExactState &E = m->exact;
    int id = -1;
    for (int i = 0; i < kTapCount; ++i)
        if (!strcmp(name, kTapName[i])) id = i;
    const bool fa = m->kind == C3_KIND_FULL_ALIGNMENT;
    if (id < 0 || (fa ? id > kTapL4 : id < kTapL4))
        return fail("c3_exact_fetch: unknown tensor \"%s\" for the %s network", name, fa ? "full-alignment" : "pileup");
    if (!E.loaded || E.last_n <= 0) return fail("c3_exact_fetch: no c3_predict_exact call since the last load");
    if (first < 0 || windows < 0 || first + windows > E.last_n)
        return fail("c3_exact_fetch: windows %lld .. %lld of %s: the last pass had %lld", (long long)first, (long long)(first + windows), name, (long long)E.last_n);
    const int64_t pw = tap_window_floats(m, id), n = windows * pw;
    if (n != n_doubles) return fail("c3_exact_fetch: %lld windows of %s are %lld doubles, caller expects %lld", (long long)windows, name, (long long)n, (long long)n_doubles);
    if (n == 0) return 0;
    const double *src = id <= 8 ? E.act[id] : id == kTapSpp ? E.spp : id == kTapL4 ? E.l4 : id == kTapLstm1 ? E.h1 : id == kTapGx2 ? E.gx2 : E.h2;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    return d2h_staged(host_out, src + first * pw, (size_t)n * sizeof(double));
}

}  // extern "C"
