// c3_exact.h -- the exact form: both networks in fp64 from end to end on the device (c3_predict_exact / c3_exact_fetch).
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
// Rows and fetched tensors leave through the pinned bounce buffer (c3_model.h d2h_staged): their layouts are the host's already.
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

// one pass: n windows at E.x -> E.y, every layer output left in the workspace
static int exact_pass(c3_model *m, hipStream_t s, int x_dtype, int64_t n) {
    ExactState &E = m->exact;
    typedef ExDense<double> DD;
    if (m->kind == C3_KIND_PILEUP) {
        const int T = m->positions;
        const int64_t M = n * T;
        // clair3/model.py:131-133: x.float(), LSTM1, LSTM2 (both bidirectional); the input projections of all steps as one contraction each
        if (x_dtype == C3_DTYPE_I32)
            TRY((exact_gemm<ExDense<int32_t>, kExBias>(s, {(const int32_t *)E.x, m->C}, E.wih[0], E.pb[0], nullptr, E.gx1, M, 1024, m->C, 1024)));
        else
            TRY((exact_gemm<ExDense<int8_t>, kExBias>(s, {(const int8_t *)E.x, m->C}, E.wih[0], E.pb[0], nullptr, E.gx1, M, 1024, m->C, 1024)));
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
                TRY((exact_gemm<ExConv<int8_t, true>, kExBiasResRelu>(s, {(const int8_t *)E.x, hh[0], ww[0], cin, hh[1], ww[1], kConvStride[0]},
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

extern "C" {

int c3_model_set_exact(c3_model *m, int enable) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
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
        TRY(exact_pass(m, s, x_dtype, n));
        TRY(d2h_staged(y_host + off * m->nout, E.y, (size_t)n * m->nout * sizeof(double), s));
        HIP_TRY(hipStreamSynchronize(s));
        E.last_n = n;
    }
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
