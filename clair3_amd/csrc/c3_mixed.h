// c3_mixed.h -- the boundary forms of a per-layer precision plan (c3_model_set_layer_precision; c3_model.h layer_f16): the fp32-MFMA form
// of a layer whose neighbours stay on their product kernels, reading and / or writing the plane activations those neighbours exchange.
//   full alignment   a named convolution as an fp32 implicit GEMM from planes to planes (c3_gemm.h ConvPlanesLoader, EPI_BIAS_RELU_PLANES /
//                    EPI_BIAS_RES_RELU_PLANES; conv1 from the int8 window, Conv1Loader), in the equalised channel units both forms share
//   pileup           the fp32 LSTM1 in front of the product projection (c3_lstm_fused.h OPT bit 4: h1 leaves as planes), the fp32
//                    projection behind the product LSTM1 (c3_gemm.h DensePlanesLoader)
// Declared in c3_forward.h; c3_model.hip includes this file last, so that these kernels are instantiated behind all the others.
// For that reason alone the launch of full alignment's fc_tail_sum_kernel (c3_tail.h, run_tail's two-launch chain) is defined here as well.
#pragma once
#include "c3_forward.h"

static int fa_conv_fp32_planes(c3_model *m, hipStream_t s, ProfScope &ps, int l, const int8_t *x, int64_t n, int cin, const int *hh, const int *ww) {
    Lane &L = lane(m);
    const int Cout = kConvCout[l];
    const int M = (int)(n * hh[l + 1] * ww[l + 1]);
    const bool res = l % 3 == 2;
    EpilogueParams ep{L.act[l], m->conv_b[l], res ? L.act[l - 2] : nullptr, Cout, 0};  // (conv_w / conv_b carry the channel exponents)
    ep.range_flag = m->range_flag;
    if (l == 0) {
        Conv1LoaderParams lp{x, (const int8_t *)m->zeros, hh[0], ww[0], cin, hh[1], ww[1]};
        ps.mfma(2.0 * ((M + 127) / 128 * 128) * 64.0 * 96.0, false);
        return launch_gemm<Conv1Loader<4>, EPI_BIAS_RELU_PLANES, 128, 64>(s, lp, m->conv_w[0], 96, M, Cout, 3, 1, ep);
    }
    ConvLoaderParams lp{L.act[l - 1], m->zeros, hh[l], ww[l], cin, hh[l + 1], ww[l + 1], kConvStride[l], cin / kBK};
    ps.mfma(2.0 * ((M + 127) / 128 * 128) * (double)Cout * 9.0 * cin, false);
    if (kConvStride[l] == 2) m->choice.s2[l == 3 ? 0 : 1] = "fp32-mfma";
    else m->choice.s1[(l / 3) * 2 + (l % 3 - 1)] = 'f', m->choice.wform[(l / 3) * 2 + (l % 3 - 1)] = '-';
    if (res) return launch_gemm<ConvPlanesLoader<4>, EPI_BIAS_RES_RELU_PLANES, 128, 64>(s, lp, m->conv_w[l], 9 * cin, M, Cout, 9 * cin / kBK, 1, ep);
    return launch_gemm<ConvPlanesLoader<4>, EPI_BIAS_RELU_PLANES, 128, 64>(s, lp, m->conv_w[l], 9 * cin, M, Cout, 9 * cin / kBK, 1, ep);
}

static int lstm1_fp32_planes(hipStream_t s, const LstmFusedParams<int8_t> &lp, int64_t n) {
    hipLaunchKernelGGL((lstm1_fused_kernel<int8_t, false, 16>), dim3((unsigned)((n + 15) / 16), 2), dim3(512), 0, s, lp);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int lstm1_fp32_planes(hipStream_t s, const LstmFusedParams<int32_t> &lp, int64_t n) {
    hipLaunchKernelGGL((lstm1_fused_kernel<int32_t, false, 16>), dim3((unsigned)((n + 15) / 16), 2), dim3(512), 0, s, lp);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int proj2_fp32_from_planes(c3_model *m, hipStream_t s, int M) {
    Lane &L = lane(m);
    DenseLoaderParams lp{L.h1, 256};
    EpilogueParams ep{L.gx2, m->proj_b[1], nullptr, 1280, 0};
    return launch_gemm<DensePlanesLoader<4>, EPI_BIAS, 128, 128>(s, lp, m->proj_w[1], 256, M, 1280, 8, 1, ep);
}

// ---- run_tail's launch of fc_tail_sum_kernel<W> (c3_tail.h): here, so that its three instantiations follow every kernel the library had
// before them and none of those moves in the code object
static int fa_tail_sum_launch(hipStream_t s, int W, const Tail2Params &tp) {
    const dim3 grid((unsigned)((tp.B + W - 1) / W), (unsigned)tp.NB);
    if (W == 4)
        hipLaunchKernelGGL(fc_tail_sum_kernel<4>, grid, dim3(512), 0, s, tp);
    else if (W == 8)
        hipLaunchKernelGGL(fc_tail_sum_kernel<8>, grid, dim3(512), 0, s, tp);
    else if (W == 16)
        hipLaunchKernelGGL(fc_tail_sum_kernel<16>, grid, dim3(512), 0, s, tp);
    else
        return fail("internal: no fc_tail_sum_kernel<%d>", W);
    return 0;
}
