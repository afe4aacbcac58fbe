// c3_forward.h -- the launch sequences of the two forward passes (clair3/model.py:130-161 Clair3_P, :377-416 Clair3_F) on a
// stream, device pointers in and out.  Per layer: the product (fp16x3 on the 16-bit matrix instructions) while layer_f16(m, layer)
// (c3_model.h: the handle is on fp16x3 and the precision plan does not name the layer), else its one fp32-MFMA form.
#pragma once
#include "c3_model.h"

// ------------------------------------------------------------------------------------------ debug taps (c3_debug.h c3_debug_tap)
// floats of one window of tap tensor `id` (plane activations take the same bytes: two fp16 pieces per value)
static int64_t tap_window_floats(const c3_model *m, int id) {
    if (id < 9) {
        int hh[10], ww[10];
        fa_geometry(m, hh, ww);
        return (int64_t)hh[id + 1] * ww[id + 1] * kConvCout[id];
    }
    switch (id) {
        case kTapSpp: return m->K4;
        case kTapL4: return m->FC;
        case kTapLstm1: return (int64_t)m->positions * 256;
        case kTapGx2: return (int64_t)m->positions * 1280;
        default: return (int64_t)m->positions * 320;
    }
}
// ---- layer records of a verified batch (c3_verify.h; c3_hostring.h sets layer_pass around its two forward passes) ----
// The product pass (1) keeps the n windows of tensor `id` in the slot's buffer, at the part's windows of the batch; the fp32 pass (2) compares
// what it just wrote at src with them, one launch per layer and part.  A tensor the product form did not produce is not compared
static int layer_tap(c3_model *m, hipStream_t s, int id, const void *src, int64_t n, bool planes) {
    HostSlot &sl = *m->layer_slot;
    const int64_t pw = tap_window_floats(m, id), first = m->tap_base - m->tap_call_off;
    if (pw % 8) return fail("internal: %s has %lld values per window, the compare kernel takes 8 at a time", kTapName[id], (long long)pw);
    if (sl.layer_dropped) return 0;
    if (m->layer_pass == 1) {
        const size_t bytes = (size_t)(m->layer_batch * pw) * sizeof(float);
        if (bytes > sl.layer_bytes[id]) {  // (the slot is free: nothing reads the smaller one)
            if (sl.layer_buf[id]) (void)hipFree(sl.layer_buf[id]);
            sl.layer_buf[id] = nullptr, sl.layer_bytes[id] = 0;
            if (hipMalloc((void **)&sl.layer_buf[id], bytes) != hipSuccess) {
                // no room for this batch's layer outputs: the prediction goes on, the batch brings no layer record (none of its layers counts)
                (void)hipGetLastError();
                sl.layer_buf[id] = nullptr, sl.layer_dropped = true, sl.layer_kept = 0;
                return 0;
            }
            sl.layer_bytes[id] = bytes;
        }
        HIP_TRY(hipMemcpyAsync(sl.layer_buf[id] + first * pw, src, (size_t)(n * pw) * sizeof(float), hipMemcpyDeviceToDevice, s));
        sl.layer_kept |= 1u << id;
        if (planes) sl.layer_planes |= 1u << id;
        return 0;
    }
    if (!(sl.layer_kept >> id & 1u)) return 0;
    if (planes) return fail("internal: the fp32 forms write no planes");
    const int blocks = (int)std::min<int64_t>(kLayerMaxBlocks, std::max<int64_t>(1, (n * (pw / 8) + kLayerThreads - 1) / kLayerThreads));
    if (sl.layer_parts[id] + blocks > sl.layer_part_stride) return fail("internal: layer partials of %s", kTapName[id]);
    LayerCompareParams cp;
    cp.a = sl.layer_buf[id] + first * pw, cp.b = (const float *)src, cp.exp = nullptr, cp.cshift = 0;
    cp.kept = m->layer_kept_count;
    cp.part = sl.layer_part + (size_t)id * sl.layer_part_stride + sl.layer_parts[id];
    cp.pw8 = (uint32_t)(pw / 8), cp.planes = (sl.layer_planes >> id & 1u) != 0;
    cp.first = (uint32_t)first, cp.n = (uint32_t)n, cp.batch = (uint32_t)m->layer_batch;
    int C = cp.planes ? (m->kind == C3_KIND_PILEUP ? 256 : kConvCout[id]) : 8;
    if (m->kind == C3_KIND_FULL_ALIGNMENT && id <= kTapSpp && !m->act_exp[std::min(id, 8)].empty()) {
        cp.exp = m->layer_exp + std::min(id, 8) * 256, C = (int)m->act_exp[std::min(id, 8)].size();
    }
    while ((8 << cp.cshift) < C) ++cp.cshift;
    if ((8 << cp.cshift) != C || pw % C) return fail("internal: %s has %d channels", kTapName[id], C);
    hipLaunchKernelGGL(layer_compare_kernel, dim3((unsigned)blocks), dim3(kLayerThreads), 0, s, cp);
    HIP_TRY(hipGetLastError());
    sl.layer_parts[id] += blocks;
    return 0;
}
// the n windows of tensor `id` that the launch just enqueued on s wrote at src: behind it on s, into the tap buffer at the part's windows
static int census_tap(c3_model *m, hipStream_t s, int id, const float *src, int64_t n);  // (c3_calibrate.h, included last like c3_mixed.h below)
static int tap(c3_model *m, hipStream_t s, int id, const void *src, int64_t n, bool planes = false) {
    if (m->census_pass) {  // 1: c3_model_calibrate, the tap buffers stay as they are; 2: the range guard's recalibrating re-run, which serves a user's taps like its sticky one
        if (planes) return fail("internal: a census pass runs the fp32 forms");
        TRY(census_tap(m, s, id, (const float *)src, n));
        if (m->census_pass == 1) return 0;
    }
    if (m->layer_pass) return layer_tap(m, s, id, src, n, planes);  // (a verified batch: no user tap is set, c3_hostring.h verify_select)
    if (!(m->tap_mask >> id & 1u)) return 0;
    const int64_t pw = tap_window_floats(m, id);
    HIP_TRY(hipMemcpyAsync(m->tap_dev[id] + m->tap_base * pw, src, (size_t)(n * pw) * sizeof(float), hipMemcpyDeviceToDevice, s));
    m->tap_written |= 1u << id;
    if (planes) m->tap_planes |= 1u << id;
    return 0;
}
// the form of this part produces no tensor `id` (it is computed inside a fused kernel)
static void tap_skip(c3_model *m, int id) {
    if (m->tap_mask >> id & 1u) m->tap_skipped |= 1u << id;
}
// at the start of a call: tap buffers for `batch` windows
static int tap_prepare(c3_model *m, int64_t batch) {
    m->tap_written = m->tap_skipped = m->tap_planes = 0;
    m->tap_n = 0, m->tap_base = 0;
    if (!m->tap_mask) return 0;
    for (int id = 0; id < kTapCount; ++id) {
        if (!(m->tap_mask >> id & 1u)) continue;
        const size_t bytes = (size_t)(batch * tap_window_floats(m, id)) * sizeof(float);
        if (bytes <= m->tap_bytes[id]) continue;
        HIP_TRY(hipDeviceSynchronize());  // (a buffer a previous call may still be copying into)
        if (m->tap_dev[id]) (void)hipFree(m->tap_dev[id]);
        m->tap_dev[id] = nullptr, m->tap_bytes[id] = 0;
        HIP_TRY(hipMalloc((void **)&m->tap_dev[id], bytes));
        m->tap_bytes[id] = bytes;
    }
    m->tap_n = batch;
    return 0;
}

// ------------------------------------------------------------------------------------------ the precision plan's boundary forms
// The fp32 forms that read or write plane activations between product layers (c3_model.h layer_f16) are defined in c3_mixed.h, which
// c3_model.hip includes LAST: their kernels are then instantiated behind every kernel of the handle without a plan, whose code keeps the
// place in the code object it has without them (clair3_amd/build.py on what moving a hot kernel costs).
static int fa_conv_fp32_planes(c3_model *m, hipStream_t s, ProfScope &ps, int l, const int8_t *x, int64_t n, int cin, const int *hh, const int *ww);
static int lstm1_fp32_planes(hipStream_t s, const LstmFusedParams<int8_t> &lp, int64_t n);  // (plain overloads: a template would be instantiated where it is used)
static int lstm1_fp32_planes(hipStream_t s, const LstmFusedParams<int32_t> &lp, int64_t n);
static int proj2_fp32_from_planes(c3_model *m, hipStream_t s, int M);
static int fa_tail_sum_launch(hipStream_t s, int W, const Tail2Params &tp);  // (fc_tail_sum_kernel<W>, c3_tail.h: defined there for its place alone)

// ------------------------------------------------------------------------------------------ FC tail (both networks)
// L4 as a split-K contraction -> splitk_reduce_selu_kernel -> fc_tail_mfma_kernel, or the latter two as one launch (c3_tail.h); the decoder
// columns behind it
static int run_tail(c3_model *m, hipStream_t s, const float *a, int64_t lda, int64_t n, float *y, const char *tag_l4,
                    const char *tag_tail) {
    Lane &L = lane(m);
    const int FC = m->FC, K4 = m->K4;
    const int nk_total = K4 / kBK;
    const int S = l4_splits(m);
    const bool l4_f16 = layer_f16(m, kLayerL4) && m->l4_wf;
    {
        ProfScope ps(m, s, tag_l4, 2.0 * n * FC * K4, 4.0 * (n * K4 + (double)FC * K4 + (double)S * n * FC));
        if (l4_f16) {  // partials carry the features' powers of two (l4_pre)
            L4Params lp{a, lda, m->l4_wf, L.part, (int)n, FC, K4 / 64, S, (int)((n + kL4BM - 1) / kL4BM), FC / kL4BN};
            ps.mfma(2.0 * lp.m_tiles * kL4BM * FC * K4 * 3, true);
            hipLaunchKernelGGL(l4_stream_kernel<0>, dim3((unsigned)(lp.m_tiles * lp.n_tiles * S)), dim3(kL4Threads), 0, s, lp);
            HIP_TRY(hipGetLastError());
        } else {
            DenseLoaderParams lp{a, lda};
            EpilogueParams ep{L.part, nullptr, nullptr, FC, n * FC};
            ps.mfma(2.0 * ((n + 127) / 128 * 128) * FC * K4, false);
            TRY((launch_gemm<DenseLoader<4>, EPI_PARTIAL, 128, 64>(s, lp, m->l4_w, K4, (int)n, FC, nk_total / S, S, ep)));
        }
    }
    {
        // full alignment's product form: the sum inside fc_tail_sum_kernel<W> (c3_tail.h).  auto: the smallest W whose grid has no more
        // workgroups than the device has CUs -- every CU streams its share of the partials once --, up to fa_tail_max_batch windows and
        // while no other batch shares the chip; otherwise workgroups would queue behind each other, and the three launches stay.  A window's
        // bits are the same in every form, so the choice may follow the batch size
        int W = 0;
        if (m->kind == C3_KIND_FULL_ALIGNMENT && FC == 256 && l4_f16 && S <= kTailSumMaxS && m->fa_tail >= 0) {
            W = m->fa_tail;
            if (!W && n <= m->fa_tail_max_batch && m->sharing == 1 && !m->lane_beside)  // (alone on the chip: c3_model.h fa_tail)
                for (const int w : {4, 8, 16})
                    if (!W && (n + w - 1) / w * m->nb <= m->wg_slots / 2) W = w;
        }
        if (m->kind == C3_KIND_FULL_ALIGNMENT) m->choice.fa_tail = W == 4 ? "fused-w4" : W == 8 ? "fused-w8" : W == 16 ? "fused-w16" : "split";
        const int64_t rows = W ? (n + W - 1) / W * 16 : (n + 15) / 16 * 16;  // tile rows the matrix instructions work on
        const double fl = 2.0 * n * (FC * 128.0 * m->nb + 128.0 * m->nout);
        ProfScope ps(m, s, tag_tail, fl, 4.0 * ((double)S * n * FC + n * m->nout));
        ps.mfma(2.0 * rows * m->nb * (FC * 128.0 + 128.0 * 48.0), false);
        Tail2Params tp{L.l4dbg, m->w5f, m->b5, m->whf, m->bh48, y, (int)n, m->nb, m->row};
        if (m->tail_fused || W) {  // the split-K sum inside the tail kernel: two launches behind the last convolution / recurrence, not three
            tp.part = L.part, tp.S = S, tp.bias4 = m->l4_b, tp.l4out = L.l4dbg;
            if (l4_f16) tp.pre = m->l4_pre, tp.post = m->l4_post;
        } else {
            ReduceParams rp{L.part, m->l4_b, L.l4dbg, (int)n, FC, S};
            if (l4_f16) rp.pre = m->l4_pre, rp.post = m->l4_post;
            hipLaunchKernelGGL(splitk_reduce_selu_kernel, dim3((unsigned)((n * FC + 255) / 256)), dim3(256), 0, s, rp);
            HIP_TRY(hipGetLastError());
        }
        const dim3 grid((unsigned)((n + 15) / 16), m->nb);
        if (W) {
            TRY(fa_tail_sum_launch(s, W, tp));
        } else if (FC == 256)
            hipLaunchKernelGGL(fc_tail_mfma_kernel<256>, grid, dim3(256), 0, s, tp);
        else
            hipLaunchKernelGGL(fc_tail_mfma_kernel<128>, grid, dim3(256), 0, s, tp);
        HIP_TRY(hipGetLastError());
        TRY(tap(m, s, kTapL4, L.l4dbg, n));
    }
    if (m->row > m->nout) {  // decoder columns behind the probabilities of every row (c3_decode.h)
        ProfScope ps(m, s, m->kind == C3_KIND_PILEUP ? "p.decode" : "fa.decode", 0.0, 4.0 * n * m->row);
        DecodeParams dp{y, m->row, nullptr, nullptr, nullptr, nullptr, y + m->nout, (int)n, m->nout == 90 ? 1 : 0};
        hipLaunchKernelGGL(outcome_maxima_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, dp);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ full alignment
// PyramidPolling geometry, clair3/model.py:250-279: the bins of the three levels clipped to the image
static int spp_bins(const c3_model *m, int H, int W, SppParams &sp) {
    sp.H = H, sp.W = W, sp.C = 256;
    int nbins = 0;
    const int pools[3] = {3, 2, 1};
    for (int pi = 0; pi < 3; ++pi) {
        const int p = pools[pi];
        const int wh_ = (H + p - 1) / p, ww_ = (W + p - 1) / p;
        const int oh_n = (H + wh_ - 1) / wh_, ow_n = (W + ww_ - 1) / ww_;
        const int pad_h = std::max((oh_n - 1) * wh_ + wh_ - H, 0), pad_w = std::max((ow_n - 1) * ww_ + ww_ - W, 0);
        const int pt = pad_h / 2, pl = pad_w / 2;
        for (int oh = 0; oh < oh_n; ++oh)
            for (int ow = 0; ow < ow_n; ++ow) {
                if (nbins >= 16) return fail("unsupported geometry: more than 16 pyramid bins");
                const int a0 = oh * wh_ - pt, a1 = a0 + wh_, c0 = ow * ww_ - pl, c1 = c0 + ww_;
                sp.h0[nbins] = (short)std::max(a0, 0), sp.h1[nbins] = (short)std::min(a1, H);
                sp.w0[nbins] = (short)std::max(c0, 0), sp.w1[nbins] = (short)std::min(c1, W);
                sp.pad[nbins] = (a0 < 0 || a1 > H || c0 < 0 || c1 > W) ? 1 : 0;
                ++nbins;
            }
    }
    if (nbins * 256 != m->K4) return fail("unsupported geometry: %d pyramid bins (L4 expects %d inputs)", nbins, m->K4);
    sp.nbins = nbins;
    return 0;
}

// magic of fast_div (c3_gemm.h) for divisor d and dividends below n: 0 = "d is 1"; fails when n * d does not fit 32 bits
static int div_magic(int d, int64_t n, uint32_t *magic) {
    if (d <= 1) return *magic = 0u, 0;
    if (n * d >= ((int64_t)1 << 32)) return fail("batch too large for the 32-bit pixel arithmetic of the convolution kernels");
    return *magic = (uint32_t)((((uint64_t)1 << 32) / (uint64_t)d) + 1), 0;
}

// the plane pipeline needs every layer packed for it and images no wider than the halo tile is sized for
static bool fa_planes_ok(const c3_model *m) {
    if (!m->f16_ok) return false;
    const uint32_t all = layer_mask_all(C3_KIND_FULL_ALIGNMENT);
    if (((m->fp32_plan | m->fp32_auto) & all) == all) return false;  // a plan of every layer IS the fp32 form (run_fa_fp32)
    int hh[10], ww[10];
    fa_geometry(m, hh, ww);
    for (int l = 1; l < 9; ++l)
        if (!m->pconv_w[l] || (kConvStride[l] == 1 && ww[l] > kPlMaxW)) return false;
    return m->C == 8 ? m->conv1_wfrag16 != nullptr : m->conv1_w16 != nullptr;
}

// The wave priority scheme of every kernel form that puts two workgroups on a CU (c3_conv3.h wave_prio_masks), chosen on the B = 256 step
// from the workgroup stamps of the probes and kept where the step's own launch got shorter by more than its run-to-run spread
// (profiles/wave_priority.txt); kPrioNone issues no s_setprio at all.
//   direct       conv3x3_planes_kernel (res1b, res3b, and whatever C3HIP_WINO leaves on it; steps = slabs of the tiles of a workgroup's walk):
//                res1b 43.4 -> 41.6 us, res3b with the pooling epilogue 44.2 -> 43.5
//   direct halo  ... with conv1 of the halo rows inside (res1a): 45.7 -> 45.3 us, inside the spread of the parent's runs -- not kept
//   wino paired  conv3x3_wino_planes_kernel (steps = slabs of a tile): res2a 36.5 -> 35.5 us, res2b 38.5 -> 37.4
// The stride-2 pair form (conv3 26.2 -> 25.9 us: inside the spread) and the two 512-thread forms that have a CU to themselves (waves 4-7 at
// priority 1: longer, or no different) keep none; their kernels carry the hook under a probe-only ABL bit.
constexpr int kPrioDirect = kPrioYoungHalf, kPrioDirectHalo = kPrioNone, kPrioWinoPaired = kPrioYoungHalf;

// activations as fp16 piece planes (c3_conv3.h), 8 convolution launches: conv1 inside res1a / res1b, the stride-2 convolutions
// on the chunk stream of c3_dense.h, the pyramid pooling as the epilogue of res3b
static int run_fa_planes(c3_model *m, hipStream_t s, const int8_t *x, int64_t n, float *y) {
    Lane &L = lane(m);
    // wave priority only while the handle has the chip to itself (the rule of the transform-waves form below): beside other handles or
    // lanes the second workgroup of a CU is somebody else's
    const bool prio_ok = m->wave_prio && std::max(m->sharing, m->lane_sharing) <= 1;
    const int cus = m->wg_slots / 2;
    m->choice.prio = 0;
    int hh[10], ww[10];
    fa_geometry(m, hh, ww);
    int cin = m->C;
    // the precision plan (c3_model.h layer_f16): a named convolution runs as an fp32 implicit GEMM that reads planes and writes planes
    // (c3_gemm.h ConvPlanesLoader, EPI_BIAS_*_PLANES), so its neighbours keep their product kernels and act[] its meaning.  conv1 lives
    // inside res1a / res1b and the pooling inside res3b: a plan that names one of those runs the unfused arrangement
    const uint32_t plan = m->fp32_plan | m->fp32_auto;
    const bool sppf_ok = m->spp_fused && !m->keep && hh[9] == 12 && ww[9] == 5 && 14 * 256 == m->K4 && !(plan & (1u << 8));
    for (int l = 0; l < 9; ++l) {
        const int Cout = kConvCout[l];
        const int M = (int)(n * hh[l + 1] * ww[l + 1]);
        // conv1 inside the first residual block (c3_conv3.h SRC8; 8-channel windows, or 9 with the dwell channel)
        const bool fuse1 = m->conv1_fused && (m->C == 8 || m->C == 9) && m->conv1_wfrag16 && !m->keep && ww[1] <= kPlMaxW && ww[0] >= 3 && !(plan & 7u);
        if (l == 0 && fuse1) {  // no launch, no conv1 planes: res1a computes its input rows, res1b its residual, from the windows
            tap_skip(m, 0);
            cin = Cout;
            continue;
        }
        double flops = 2.0 * M * Cout * 9.0 * cin;
        double bytes = (l == 0 ? 1.0 : 4.0) * n * hh[l] * ww[l] * cin + 4.0 * M * Cout * (l % 3 == 2 ? 2 : 1) + 4.0 * Cout * 9.0 * cin;
        if (fuse1 && l == 1) flops += 2.0 * M * 64.0 * 9.0 * m->C, bytes += 1.0 * n * hh[0] * ww[0] * m->C - 4.0 * M * 64;  // conv1's algorithmic work rides here
        if (fuse1 && l == 2) bytes += 1.0 * n * hh[0] * ww[0] * m->C - 4.0 * M * 64;  // residual from the windows, not from conv1 planes
        ProfScope ps(m, s, kFaLayerTag[l], flops, bytes);
        if (plan >> l & 1u) {  // the fp32 form between planes (c3_mixed.h)
            TRY(fa_conv_fp32_planes(m, s, ps, l, x, n, cin, hh, ww));
        } else if (l == 0 && cin == 8) {
            ps.mfma(2.0 * ((M + 31) / 32 * 32) * 64.0 * 80.0 * 2, true);
            Conv1F16Params cp;
            cp.x = x, cp.wfrag = reinterpret_cast<const uint32_t *>(m->conv1_wfrag16), cp.bias = m->conv_b[0], cp.out = L.act[0];
            cp.range_flag = m->range_flag, cp.post = m->conv1_post;
            cp.B = (int)n, cp.H = hh[0], cp.W = ww[0], cp.OH = hh[1], cp.OW = ww[1], cp.M = M, cp.groups = (M + 31) / 32;
            const int grid = std::min((cp.groups + 3) / 4, m->wg_slots);
            hipLaunchKernelGGL(conv1_i8_f16_kernel<true>, dim3(grid), dim3(256), 0, s, cp);
            HIP_TRY(hipGetLastError());
        } else if (l == 0) {
            ps.mfma(2.0 * ((M + 127) / 128 * 128) * 64.0 * 96.0 * 3, true);
            Conv1LoaderParams lp{x, (const int8_t *)m->zeros, hh[0], ww[0], cin, hh[1], ww[1]};
            EpilogueParams ep{L.act[0], m->conv_b[0], nullptr, Cout, 0};
            ep.post = m->conv1_w16_post, ep.range_flag = m->range_flag;
            TRY((launch_gemm<Conv1Loader<4>, EPI_BIAS_RELU_PLANES, 128, 64, 2>(s, lp, m->conv_w[0], 96, M, Cout, 3, 1, ep, m->conv1_w16)));
        } else if (kConvStride[l] == 2) {
            S2ConvParams sp;
            sp.a = L.act[l - 1], sp.wf = m->pconv_w[l], sp.bias = m->conv_b[l], sp.post = m->pconv_post[l], sp.c = L.act[l], sp.range_flag = m->range_flag;
            sp.M = M, sp.N = Cout, sp.NK = 9 * cin / 64, sp.tiles_n = Cout / kS2BN, sp.tiles = (M + kS2BM - 1) / kS2BM * sp.tiles_n;
            sp.Hin = hh[l], sp.Win = ww[l], sp.Cin = cin, sp.Ho = hh[l + 1], sp.Wo = ww[l + 1];
            TRY(div_magic(hh[l + 1] * ww[l + 1], (int64_t)M + 2 * kS2BM, &sp.mg_hw));
            TRY(div_magic(ww[l + 1], hh[l + 1] * ww[l + 1], &sp.mg_w));
            ps.mfma(2.0 * ((M + kS2BM - 1) / kS2BM * kS2BM) * (double)Cout * 9.0 * cin * 3, true);
            // more tiles than CUs: two 512-thread workgroups (66 KB of LDS, 128 registers a lane) per CU; otherwise one, with twice the registers
            const bool pair = sp.tiles > m->wg_slots / 2;
            m->choice.s2[l == 3 ? 0 : 1] = pair ? "two-workgroups-per-cu" : "one-workgroup-per-cu";
            int g = sp.tiles;
            const int slots = pair ? m->wg_slots : m->wg_slots / 2, unit = 8 * sp.tiles_n;
            if (g > slots) g = std::max(unit, slots / unit * unit);
            if (pair) hipLaunchKernelGGL((conv3x3_s2_planes_kernel<0, true>), dim3(g), dim3(kS2Threads), 0, s, sp);
            else
                hipLaunchKernelGGL((conv3x3_s2_planes_kernel<0, false>), dim3(g), dim3(kS2Threads), 0, s, sp);
            HIP_TRY(hipGetLastError());
        } else {
            const bool res = l % 3 == 2;
            PlaneConvParams cp;
            cp.x = L.act[l - 1], cp.wf = m->pconv_w[l], cp.bias = m->conv_b[l], cp.res = res ? L.act[l - 2] : nullptr, cp.out = L.act[l];
            cp.range_flag = m->range_flag, cp.post = m->pconv_post[l], cp.pre = m->pconv_pre[l];
            cp.M = M, cp.H = hh[l], cp.W = ww[l];
            TRY(div_magic(hh[l] * ww[l], (int64_t)M + 2 * kPlBM, &cp.mg_hw));
            TRY(div_magic(ww[l], hh[l] * ww[l], &cp.mg_w));
            const int tiles_m = (M + kPlBM - 1) / kPlBM;
            cp.tiles = tiles_m * (Cout / 64);
            const bool src8 = fuse1 && (l == 1 || l == 2);
            // PyramidPolling as the epilogue of the last convolution (c3_conv3.h SPPF): 12 x 5 windows, two whole windows per tile
            const bool sppf = l == 8 && sppf_ok;
            constexpr int wpt = kPlBM / 60;  // windows per tile
            if (sppf) {
                cp.spp = L.spp;
                cp.tiles = (int)((n + wpt - 1) / wpt) * (Cout / 64);
            }
            if (src8) {
                cp.x8 = x, cp.c1w = reinterpret_cast<const uint32_t *>(m->conv1_wfrag16), cp.c1b = m->conv_b[0], cp.c1post = m->conv1_post, cp.Hin = hh[0], cp.Win = ww[0];
                if (l == 1) cp.x = nullptr;
                else cp.res = nullptr;
            }
            // SRC8: + conv1 for the halo rows of a tile in groups of 32 (res1a) / the tile's own pixels (res1b), two piece products of
            // K = 80 (96 for 9 channels)
            const double tiles_x = sppf ? (double)((n + wpt - 1) / wpt) : (double)tiles_m;  // pixel tiles the launch really runs
            const int c1_rows = l == 1 ? (kPlBM + 2 * ww[l] + 2 + 31) / 32 * 32 : kPlBM;
            ps.mfma(2.0 * tiles_x * kPlBM * (double)Cout * 9.0 * cin * 3 + (src8 ? 2.0 * tiles_m * c1_rows * 64.0 * (m->C == 8 ? 80.0 : 96.0) * 2 : 0.0), true);
            m->choice.s1[(l / 3) * 2 + (l % 3 - 1)] = 'd';
            m->choice.wform[(l / 3) * 2 + (l % 3 - 1)] = '-';
            // F(2,3) along H (c3_conv3w.h) for the plain plane-to-plane layers: 12 instead of 18 groups of piece products per output
            // pair.  Not where conv1 is computed inside the kernel (res1a / res1b) or the pyramid pooling is its epilogue (res3b):
            // those stay on the direct kernel.  C3HIP_WINO: 0 none, 1 the 64- / 128-channel ones, 2 (default) every plain one -- same-box
            // A/B of the whole step in round 5 (profiles/r05_e_ab_wino_step*.txt): B = 256 707 k -> 729 k windows/s (res2a / res2b 48.3 / 50.3
            // -> 41.7 / 43.8 us; res3a unchanged THEN: 244 tiles = one workgroup per CU, which is what the transform-waves form below is
            // for), B = 1000 774 k -> 804 k (res3a 172 -> 148.5 us as well).
            const bool wino_layer = m->wino >= 2 || (m->wino == 1 && (Cout == 64 || Cout == 128));
            if (wino_layer && !src8 && !sppf && m->wconv_w[l]) {
                WinoConvParams wp;
                wp.x = L.act[l - 1], wp.wf = m->wconv_w[l], wp.bias = m->conv_b[l], wp.post = m->wconv_post[l];
                wp.res = res ? L.act[l - 2] : nullptr, wp.out = L.act[l], wp.range_flag = m->range_flag;
                wp.M = M, wp.H = hh[l], wp.W = ww[l], wp.Hj = (hh[l] + 1) / 2, wp.Mp = (int)(n * wp.Hj * ww[l]);
                TRY(div_magic(wp.Hj * ww[l], (int64_t)wp.Mp + 2 * kWTM, &wp.mg_hjw));
                TRY(div_magic(ww[l], wp.Hj * ww[l], &wp.mg_w));
                const int tiles_w = (wp.Mp + kWTM - 1) / kWTM;
                wp.tiles = tiles_w * (Cout / 64);
                ps.mfma(2.0 * tiles_w * kWRows * (double)Cout * 12.0 * cin * 3, true);
                // Launches that leave the second workgroup slot of every CU empty take the transform-waves form (c3_conv3w.h): one
                // 512-thread workgroup per tile, whose waves 4-7 transform the next slab under the tap loop of waves 0-3; rows are
                // bit-identical.  It takes a whole CU's LDS, so not where the handle is TOLD or KNOWS that other batches need the CUs:
                // `beside` is the caller's hint (c3_model_set_sharing: several handles feed the chip) or the ring's own finding that this
                // batch and those in its other lanes together oversubscribe the CUs on half tiles (c3_hostring.h LaneSharing: beyond
                // ~1000 windows in flight).  Smaller batches in three lanes (3 x 256 windows) keep beside == 1 and each takes the form.
                // kWtMaxTiles: the tile count up to which it is taken, in CUs.  Same box, builds alternated (profiles/wino_transform_waves.txt):
                // res3a at B = 256 (244 tiles) 45.0 -> 37.1 us, the step 744 k -> 764 k windows/s; with 2 (res2a / res2b, 440 tiles in two
                // rounds) 42.1 / 40.1 -> 41.2 / 40.3 us and a step inside the run-to-run spread of 1: not taken.
                constexpr int kWtMaxTiles = 1;
                const int beside = std::max(m->sharing, m->lane_sharing);
                const bool tw = wp.tiles <= kWtMaxTiles * (m->wg_slots / 2) && beside <= 1;
                m->choice.wform[(l / 3) * 2 + (l % 3 - 1)] = tw ? 't' : 'p';
                int gw = wp.tiles;
                const int wslots = m->wg_slots, wunit = 8 * (Cout / 64);
                if (gw > wslots) gw = std::max(wunit, wslots / wunit * wunit);
                const dim3 wgrid(gw), wblock(tw ? kWtThreads : kPlThreads);
                if (const int scheme = prio_ok && !tw && gw > cus ? kPrioWinoPaired : kPrioNone) {
                    wave_prio_masks(scheme, cin / 32, wp.prio), wp.cus = cus;
                    m->choice.prio |= 1u << l;
                }
                if (tw && Cout == 64) {
                    if (res) hipLaunchKernelGGL((conv3x3_wino_tw_kernel<64, true>), wgrid, wblock, 0, s, wp);
                    else hipLaunchKernelGGL((conv3x3_wino_tw_kernel<64, false>), wgrid, wblock, 0, s, wp);
                } else if (tw && Cout == 128) {
                    if (res) hipLaunchKernelGGL((conv3x3_wino_tw_kernel<128, true>), wgrid, wblock, 0, s, wp);
                    else hipLaunchKernelGGL((conv3x3_wino_tw_kernel<128, false>), wgrid, wblock, 0, s, wp);
                } else if (tw) {
                    if (res) hipLaunchKernelGGL((conv3x3_wino_tw_kernel<256, true>), wgrid, wblock, 0, s, wp);
                    else hipLaunchKernelGGL((conv3x3_wino_tw_kernel<256, false>), wgrid, wblock, 0, s, wp);
                } else if (Cout == 64) {
                    if (res) hipLaunchKernelGGL((conv3x3_wino_planes_kernel<64, true>), wgrid, wblock, 0, s, wp);
                    else hipLaunchKernelGGL((conv3x3_wino_planes_kernel<64, false>), wgrid, wblock, 0, s, wp);
                } else if (Cout == 128) {
                    if (res) hipLaunchKernelGGL((conv3x3_wino_planes_kernel<128, true>), wgrid, wblock, 0, s, wp);
                    else hipLaunchKernelGGL((conv3x3_wino_planes_kernel<128, false>), wgrid, wblock, 0, s, wp);
                } else {
                    if (res) hipLaunchKernelGGL((conv3x3_wino_planes_kernel<256, true>), wgrid, wblock, 0, s, wp);
                    else hipLaunchKernelGGL((conv3x3_wino_planes_kernel<256, false>), wgrid, wblock, 0, s, wp);
                }
                HIP_TRY(hipGetLastError());
                TRY(tap(m, s, l, L.act[l], n, true));
                m->choice.s1[(l / 3) * 2 + (l % 3 - 1)] = 'w';
                cin = Cout;
                continue;
            }
            // persistent: one workgroup per tile when they all fit (two 256-thread workgroups, <= 70 KB of LDS each, per CU), else as
            // many as fit, rounded down so that a workgroup's tiles share their column tile (c3_conv3.h)
            int g = cp.tiles;
            const int slots = m->wg_slots, unit = 8 * (Cout / 64);
            if (g > slots) g = std::max(unit, slots / unit * unit);
            const dim3 grid(g), block(kPlThreads);
            if (const int scheme = !(prio_ok && g > cus) ? kPrioNone : src8 && l == 1 ? kPrioDirectHalo : kPrioDirect) {
                wave_prio_masks(scheme, (cp.tiles + g - 1) / g * (Cout / 64), cp.prio), cp.cus = cus;
                m->choice.prio |= 1u << l;
            }
            if (Cout == 64 && src8 && m->C == 9) {
                if (res) hipLaunchKernelGGL((conv3x3_planes_kernel<64, true, 0, 2, false, 9>), grid, block, 0, s, cp);
                else hipLaunchKernelGGL((conv3x3_planes_kernel<64, false, 0, 1, false, 9>), grid, block, 0, s, cp);
            } else if (Cout == 64 && src8) {
                if (res) hipLaunchKernelGGL((conv3x3_planes_kernel<64, true, 0, 2>), grid, block, 0, s, cp);
                else hipLaunchKernelGGL((conv3x3_planes_kernel<64, false, 0, 1>), grid, block, 0, s, cp);
            } else if (Cout == 64) {
                if (res) hipLaunchKernelGGL((conv3x3_planes_kernel<64, true>), grid, block, 0, s, cp);
                else hipLaunchKernelGGL((conv3x3_planes_kernel<64, false>), grid, block, 0, s, cp);
            } else if (Cout == 128) {
                if (res) hipLaunchKernelGGL((conv3x3_planes_kernel<128, true>), grid, block, 0, s, cp);
                else hipLaunchKernelGGL((conv3x3_planes_kernel<128, false>), grid, block, 0, s, cp);
            } else {
                if (sppf) hipLaunchKernelGGL((conv3x3_planes_kernel<256, true, 0, 0, true>), grid, block, 0, s, cp);
                else if (res) hipLaunchKernelGGL((conv3x3_planes_kernel<256, true>), grid, block, 0, s, cp);
                else hipLaunchKernelGGL((conv3x3_planes_kernel<256, false>), grid, block, 0, s, cp);
            }
            HIP_TRY(hipGetLastError());
            if (sppf) {  // the epilogue pooled the tiles: spp written, no act8
                tap_skip(m, 8);
                TRY(tap(m, s, kTapSpp, L.spp, n));
                cin = Cout;
                continue;
            }
        }
        TRY(tap(m, s, l, L.act[l], n, true));
        cin = Cout;
    }
    if (!sppf_ok) {
        ProfScope ps(m, s, "fa.spp", 0.0, 4.0 * n * (hh[9] * ww[9] * 256.0 + m->K4));
        if (hh[9] == 12 && ww[9] == 5) {
            if (14 * 256 != m->K4) return fail("unsupported geometry: L4 expects %d inputs", m->K4);
            const int grid = (int)std::min<int64_t>(n, 8192);
            hipLaunchKernelGGL((spp_planes_fixed_kernel<12, 5>), dim3(grid), dim3(256), 0, s, (const void *)L.act[8], L.spp, (int)n, 256);
        } else {
            SppParams sp;
            TRY(spp_bins(m, hh[9], ww[9], sp));
            sp.in = L.act[8], sp.out = L.spp, sp.B = (int)n;
            const int64_t total = n * m->K4;
            const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
            hipLaunchKernelGGL(spp_planes_kernel, dim3(grid), dim3(256), 0, s, sp);
        }
        HIP_TRY(hipGetLastError());
        TRY(tap(m, s, kTapSpp, L.spp, n));
    }
    L.last_planes = true;
    return run_tail(m, s, L.spp, m->K4, n, y, "fa.l4", "fa.tail");
}

// The fp32 form of the full-alignment network (range-guard fallback, C3HIP_FP32=1, geometries the plane kernels are not
// sized for): fp32 NHWC activations, every convolution an implicit GEMM on v_mfma_f32_32x32x2_f32 (c3_gemm.h ConvLoader /
// Conv1Loader), pooling and tail on fp32.
static int run_fa_fp32(c3_model *m, hipStream_t s, const int8_t *x, int64_t n, float *y) {
    Lane &L = lane(m);
    L.last_planes = false;
    int hh[10], ww[10];
    fa_geometry(m, hh, ww);
    int cin = m->C;
    for (int l = 0; l < 9; ++l) {
        const int Cout = kConvCout[l];
        const int M = (int)(n * hh[l + 1] * ww[l + 1]);
        const double flops = 2.0 * M * Cout * 9.0 * cin;
        const double bytes = (l == 0 ? 1.0 : 4.0) * n * hh[l] * ww[l] * cin + 4.0 * M * Cout * (l % 3 == 2 ? 2 : 1) + 4.0 * Cout * 9.0 * cin;
        ProfScope ps(m, s, kFaLayerTag[l], flops, bytes);
        const bool res = l % 3 == 2;
        EpilogueParams ep{L.act[l], m->conv_b[l], res ? L.act[l - 2] : nullptr, Cout, 0};
        if (l == 0) {
            Conv1LoaderParams lp{x, (const int8_t *)m->zeros, hh[0], ww[0], cin, hh[1], ww[1]};
            ps.mfma(2.0 * ((M + 127) / 128 * 128) * 64.0 * 96.0, false);
            TRY((launch_gemm<Conv1Loader<4>, EPI_BIAS_RELU, 128, 64>(s, lp, m->conv_w[0], 96, M, Cout, 3, 1, ep)));
        } else {
            ConvLoaderParams lp{L.act[l - 1], m->zeros, hh[l], ww[l], cin, hh[l + 1], ww[l + 1], kConvStride[l], cin / kBK};
            const int nk = 9 * cin / kBK;
            const int64_t ldb = 9 * cin;
            ps.mfma(2.0 * ((M + 127) / 128 * 128) * (double)Cout * 9.0 * cin, false);
            if (res)
                TRY((launch_gemm<ConvLoader<4>, EPI_BIAS_RES_RELU, 128, 64>(s, lp, m->conv_w[l], ldb, M, Cout, nk, 1, ep)));
            else
                TRY((launch_gemm<ConvLoader<4>, EPI_BIAS_RELU, 128, 64>(s, lp, m->conv_w[l], ldb, M, Cout, nk, 1, ep)));
        }
        TRY(tap(m, s, l, L.act[l], n));
        cin = Cout;
    }
    {
        SppParams sp;
        TRY(spp_bins(m, hh[9], ww[9], sp));
        sp.in = L.act[8], sp.out = L.spp, sp.B = (int)n;
        ProfScope ps(m, s, "fa.spp", 0.0, 4.0 * n * (hh[9] * ww[9] * 256.0 + m->K4));
        const int64_t total = n * m->K4;
        const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
        hipLaunchKernelGGL(spp_kernel, dim3(grid), dim3(256), 0, s, sp);
        HIP_TRY(hipGetLastError());
        TRY(tap(m, s, kTapSpp, L.spp, n));
    }
    return run_tail(m, s, L.spp, m->K4, n, y, "fa.l4", "fa.tail");
}

static int run_fa(c3_model *m, hipStream_t s, const int8_t *x, int64_t n, float *y) {
    if (fa_planes_ok(m)) {
        m->choice.fa = "planes-f16x3";
        return run_fa_planes(m, s, x, n, y);
    }
    m->choice.fa = "fp32-mfma", m->choice.s2[0] = m->choice.s2[1] = "-";
    return run_fa_fp32(m, s, x, n, y);
}

// ------------------------------------------------------------------------------------------ pileup
// LSTM1 (input projection fused into the recurrence, h1 out as planes) -> LSTM2 projection (weights resident in registers) ->
// LSTM2 recurrence -> tail.  With `starts` the windows are gathered out of one region matrix (c3_predict_pileup_region).
template <typename T>
static int run_pileup_t(c3_model *m, hipStream_t s, const T *x, int64_t n, float *y, const int32_t *starts = nullptr) {
    Lane &L = lane(m);
    const int Tn = m->positions;
    const int M = (int)(n * Tn);
    // int8 windows feed the fp16 projection fragments (counts are exact in fp16); int32 windows keep an fp32 projection inside
    // the fp16x3 recurrence kernel
    const bool l1_f16 = layer_f16(m, kLayerLstm1) && m->whh16[0] && (sizeof(T) != 1 || m->l1_wih16);
    const int beside = std::max(m->sharing, m->lane_sharing);  // other batches on the chip: the caller's handles, or this handle's other lanes (c3_model.h)
    // h1 leaves LSTM1 as fp16 piece planes for c3_dense.h.  Under a precision plan (c3_model.h layer_f16) the product LSTM1 keeps writing
    // them whatever reads them -- an fp32 projection then reads planes (c3_gemm.h DensePlanesLoader), so that LSTM1 runs the very kernel and
    // tile shape it runs without a plan -- and an fp32 LSTM1 in front of the product projection writes them too (c3_lstm_fused.h OPT bit 4)
    const bool p2_f16 = layer_f16(m, kLayerProj2) && m->proj2_pw;
    const bool h1_planes = l1_f16 ? m->proj2_pw != nullptr : p2_f16 && ((m->fp32_plan | m->fp32_auto) & kLayerLstm1);
    L.last_planes = h1_planes;
    {
        ProfScope ps(m, s, "p.lstm1", 2.0 * M * 1024.0 * m->C + 2.0 * M * 2.0 * 512.0 * 128.0, sizeof(T) * (double)M * m->C + 4.0 * M * 256.0);
        // half tiles (8 windows per workgroup, c3_lstm_fused.h OPT bit 2) while the full tiles would leave half the CUs without a
        // workgroup (<= 1024 windows on 256 CUs; beyond that two half tiles share a CU and take twice as long: 1100 windows 94 us
        // against 60 us on full tiles)
        const bool half1 = l1_f16 && m->half_tiles && beside <= 1 && h1_planes && sizeof(T) == 1 && 2 * ((n + 15) / 16) <= m->wg_slots / 4;
        const double tiles = (double)(half1 ? (n + 7) / 8 * 16 : (n + 15) / 16 * 16) * Tn * 2;  // (window, step, direction) rows of the 16-row tiles
        // recurrent part 512 x 128 as fp16x3 (or fp32); input part: int8 windows 512 x 32 against two weight pieces, else 512 x 20 fp32
        ps.mfma(l1_f16 ? tiles * 2.0 * 512 * (128 * 3 + (sizeof(T) == 1 ? 32 * 2 : 0)) : tiles * 2.0 * 512 * (128 + 20), l1_f16);
        LstmFusedParams<T> lp{x, starts, m->l1_wih, m->l1_bias, m->whh[0], reinterpret_cast<const uint32_t *>(m->l1_wih16), L.h1, (int)n, Tn, m->C};
        const dim3 grid((unsigned)((n + 15) / 16), 2);
        if (l1_f16) {
            lp.whh = m->whh16[0];
            if (h1_planes) lp.hplanes = L.h1;
            m->choice.lstm1 = half1 ? "fused-f16x3-half-tiles" : "fused-f16x3-full-tiles";
            bool launched = false;
            if constexpr (sizeof(T) == 1) {
                if (half1) {
                    hipLaunchKernelGGL((lstm1_fused_kernel<T, true, 7>), dim3((unsigned)((n + 7) / 8), 2), dim3(512), 0, s, lp);
                    launched = true;
                }
            }
            if (!launched) {
                if (h1_planes) hipLaunchKernelGGL((lstm1_fused_kernel<T, true, 3>), grid, dim3(512), 0, s, lp);
                else hipLaunchKernelGGL((lstm1_fused_kernel<T, true>), grid, dim3(512), 0, s, lp);
            }
        } else if (h1_planes) {
            lp.hplanes = L.h1;
            m->choice.lstm1 = "fused-fp32-mfma-planes";
            TRY(lstm1_fp32_planes(s, lp, n));
        } else {
            m->choice.lstm1 = "fused-fp32-mfma";
            hipLaunchKernelGGL(lstm1_fused_kernel<T>, grid, dim3(512), 0, s, lp);
        }
        HIP_TRY(hipGetLastError());
        TRY(tap(m, s, kTapLstm1, L.h1, n, h1_planes));
    }
    {
        ProfScope ps(m, s, "p.proj2", 2.0 * M * 1280.0 * 256.0, 4.0 * M * (256.0 + 1280.0));
        ps.mfma(2.0 * ((M + 127) / 128 * 128) * 1280.0 * 256.0 * (h1_planes && p2_f16 ? 3 : 1), h1_planes && p2_f16);
        if (!p2_f16 && h1_planes) {  // the fp32 form behind a product LSTM1
            m->choice.proj2 = "fp32-mfma";
            TRY(proj2_fp32_from_planes(m, s, M));
        } else if (h1_planes && m->proj2_pwr && (M + kWrBM - 1) / kWrBM >= 2 * 8 * std::max(1, m->wg_slots / 16 / (1280 / kWrBN))) {
            // weights resident in registers (c3_dense.h): 8 XCDs x lanes x 5 column tiles of workgroups, each walking the row tiles of its lane
            DenseWresParams wp;
            wp.a = L.h1, wp.w = m->proj2_pwr, wp.bias = m->proj_b[1], wp.c = L.gx2, wp.post_scale = m->proj2_post_scale;
            wp.M = M, wp.N = 1280, wp.tiles_m = (M + kWrBM - 1) / kWrBM, wp.tiles_n = 1280 / kWrBN;
            wp.lanes_per_xcd = std::max(1, m->wg_slots / 16 / wp.tiles_n);  // CUs per XCD / column tiles (32 / 5 = 6)
            // beside other handles half as many, twice as long workgroups: 120 of them leave room for the 128 of another batch's
            // LSTM launch (three batches in flight 5.46 M -> 5.59 M windows/s; alone 4.9 M -> 4.3 M, hence the caller's hint)
            if (beside > 1) wp.lanes_per_xcd = std::max(1, wp.lanes_per_xcd / 2);
            m->choice.proj2 = beside > 1 ? "weights-resident-half-grid" : "weights-resident";
            hipLaunchKernelGGL(dense_planes_wres_kernel<0>, dim3(8 * wp.lanes_per_xcd * wp.tiles_n), dim3(kDnThreads), 0, s, wp);
            HIP_TRY(hipGetLastError());
        } else if (h1_planes) {  // batches below ~190 windows: fewer than two row tiles per lane
            DensePlanesParams dp;
            dp.a = L.h1, dp.w = m->proj2_pw, dp.bias = m->proj_b[1], dp.c = L.gx2, dp.post = m->proj2_post;
            dp.M = M, dp.N = 1280, dp.K = 256, dp.tiles_n = 1280 / kDnBN, dp.tiles = ((M + kDnBM - 1) / kDnBM) * dp.tiles_n;
            m->choice.proj2 = "128x128-chunk-stream";
            hipLaunchKernelGGL(dense_planes_pipe_kernel<0>, dim3(std::min(dp.tiles, m->wg_slots / 2)), dim3(kDnThreads), 0, s, dp);
            HIP_TRY(hipGetLastError());
        } else {
            DenseLoaderParams lp{L.h1, 256};
            EpilogueParams ep{L.gx2, m->proj_b[1], nullptr, 1280, 0};
            m->choice.proj2 = "fp32-mfma";
            TRY((launch_gemm<DenseLoader<4>, EPI_BIAS, 128, 128>(s, lp, m->proj_w[1], 256, M, 1280, 8, 1, ep)));
        }
        TRY(tap(m, s, kTapGx2, L.gx2, n));
    }
    {
        ProfScope ps(m, s, "p.lstm2", 2.0 * M * 2.0 * 640.0 * 160.0, 4.0 * M * (1280.0 + 320.0));
        const bool l2_f16 = layer_f16(m, kLayerLstm2) && m->whh16[1];
        const bool half2 = l2_f16 && m->half_tiles && beside <= 1 && 2 * ((n + 15) / 16) <= m->wg_slots / 4;
        ps.mfma((double)(half2 ? (n + 7) / 8 * 16 : (n + 15) / 16 * 16) * Tn * 2 * 2.0 * 640 * 160 * (l2_f16 ? 3 : 1), l2_f16);
        Lstm2Params lp{L.gx2, m->whh[1], L.h2, (int)n, Tn, 1280};
        if (l2_f16) {
            lp.whh = m->whh16[1];
            m->choice.lstm2 = half2 ? "f16x3-half-tiles" : "f16x3-full-tiles";
            if (half2) hipLaunchKernelGGL((lstm_recurrent_kernel_v2<160, true, 4>), dim3((unsigned)((n + 7) / 8), 2), dim3(512), 0, s, lp);
            else hipLaunchKernelGGL((lstm_recurrent_kernel_v2<160, true>), dim3((unsigned)((n + 15) / 16), 2), dim3(512), 0, s, lp);
        } else {
            m->choice.lstm2 = "fp32-mfma";
            hipLaunchKernelGGL(lstm_recurrent_kernel_v2<160>, dim3((unsigned)((n + 15) / 16), 2), dim3(512), 0, s, lp);
        }
        HIP_TRY(hipGetLastError());
        TRY(tap(m, s, kTapLstm2, L.h2, n));
    }
    return run_tail(m, s, L.h2, m->K4, n, y, "p.l4", "p.tail");
}

// ------------------------------------------------------------------------------------------ both
// With `depth` (pileup, int32 counts; one per window, device): the reference's rescaling of very deep windows (c3_rescale.h) as a pre-pass
// into the lane's buffer of sliced windows, then the int32 forms on that buffer -- x (and the region matrix behind `starts`) stays as it came.
// With `rows` (full alignment; one table entry per window, device): x holds the occupied rows of the windows and the pre-pass of
// c3_expand.h writes the dense windows of every micro-batch into the lane's buffer in front of the unchanged forward pass.
static int forward_device(c3_model *m, hipStream_t s, const void *x, int x_dtype, int64_t batch, float *y,
                          const int32_t *starts = nullptr, const int32_t *depth = nullptr, const ExpandEntry *rows = nullptr) {
    if (!m->loaded) return fail("model has no weights: call c3_model_load first");
    if (batch < 0) return fail("negative batch");
    if (batch == 0) return 0;
    if (m->kind == C3_KIND_FULL_ALIGNMENT && x_dtype != C3_DTYPE_I8)
        return fail("full-alignment windows must be int8 (got dtype %d)", x_dtype);
    if (m->kind == C3_KIND_PILEUP && x_dtype != C3_DTYPE_I8 && x_dtype != C3_DTYPE_I32)
        return fail("pileup windows must be int8 or int32 (got dtype %d)", x_dtype);
    if (depth && (m->kind != C3_KIND_PILEUP || x_dtype != C3_DTYPE_I32)) return fail("internal: depths need int32 pileup counts");
    TRY(ensure_workspace(m, batch));
    if (depth) TRY(ensure_rescale_buf(m));
    if (rows && (m->kind != C3_KIND_FULL_ALIGNMENT || x_dtype != C3_DTYPE_I8)) return fail("internal: rows need int8 full-alignment windows");
    if (rows) TRY(ensure_expand_buf(m));
    if (!m->tap_call) TRY(tap_prepare(m, batch));
    const int64_t wbytes = c3_model_window_bytes(m, x_dtype);
    Lane &L = lane(m);
    for (int64_t off = 0; off < batch; off += L.cap) {
        const int64_t n = std::min<int64_t>(L.cap, batch - off);
        const char *xp = starts ? (const char *)x : (const char *)x + off * wbytes;  // region matrix is shared
        const int32_t *sp = starts ? starts + off : nullptr;
        float *yp = y + off * m->row;
        m->tap_base = m->tap_call_off + off;
        if (m->kind == C3_KIND_FULL_ALIGNMENT && rows) {
            {
                ExpandParams ep{(const int8_t *)x, rows + off, L.xe, (int)n, m->positions * m->C, (int)wbytes};
                ProfScope ps(m, s, "fa.expand", 0.0, 2.0 * (double)n * (double)wbytes);
                if (ep.row_bytes % 8 == 0) hipLaunchKernelGGL(expand_rows_kernel<8>, dim3((unsigned)n), dim3(kExpandThreads), 0, s, ep);
                else hipLaunchKernelGGL(expand_rows_kernel<1>, dim3((unsigned)n), dim3(kExpandThreads), 0, s, ep);
                HIP_TRY(hipGetLastError());
            }
            TRY(run_fa(m, s, L.xe, n, yp));
        } else if (m->kind == C3_KIND_FULL_ALIGNMENT) TRY(run_fa(m, s, (const int8_t *)xp, n, yp));
        else if (x_dtype == C3_DTYPE_I8) TRY(run_pileup_t<int8_t>(m, s, (const int8_t *)xp, n, yp, sp));
        else if (depth) {
            {
                const int TC = m->positions * m->C;
                ProfScope ps(m, s, "p.rescale", 0.0, 2.0 * sizeof(int32_t) * (double)n * TC);
                RescaleParams rp{(const int32_t *)xp, sp, depth + off, L.xr, (int)n, TC, m->C, m->max_depth};
                const dim3 grid((unsigned)((n + kRescaleWindows - 1) / kRescaleWindows));
                if (m->C % 2 == 0) hipLaunchKernelGGL(rescale_windows_kernel<2>, grid, dim3(kRescaleThreads), 0, s, rp);
                else hipLaunchKernelGGL(rescale_windows_kernel<1>, grid, dim3(kRescaleThreads), 0, s, rp);
                HIP_TRY(hipGetLastError());
            }
            TRY(run_pileup_t<int32_t>(m, s, L.xr, n, yp));
        } else TRY(run_pileup_t<int32_t>(m, s, (const int32_t *)xp, n, yp, sp));
        L.last_n = n;
    }
    return 0;
}
