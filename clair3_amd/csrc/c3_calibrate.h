// c3_calibrate.h -- full alignment: channel exponents calibrated from observed activations (c3_model_calibrate and the entries around it,
// include/c3hip.h; DESIGN.md 1 Range).  Channel equalisation at load time (c3_pack.h fa_channel_exps) reads gamma and beta only; a checkpoint
// whose BatchNorm statistics do not predict its activations meets the range guard instead (c3_gemm.h kF16Range) and runs on the fp32 forms
// from then on.  Here the activations are measured on a sample of the job's own windows:
//   census   the windows run on the fp32 forms (run_fa_fp32: no range limit), and behind every convolution channel_absmax_kernel takes
//            max |x| per channel of the layer's output (c3_forward.h tap, census_pass).  Read out in the checkpoint's units, x * 2^-act_exp
//   rule     per channel group of FaChannelExps: how many powers of two a channel's exponent has to come DOWN for what was seen to stay
//            below 2^cap, and a group shift (the lower median of those) for the channels the sample happened not to excite.  Never up
//   load     c3_model_load packs with k = k0 - lowering wherever it used k0: exact powers of two, the rows of the checkpoint as given
//   online   the range guard's own fp32 re-run is such a pass over exactly the windows that tripped it: under the policy C3_RANGE_RECALIBRATE
//            (c3_model_set_range_policy; the end of this file) a trip takes the census, solves, packs again and the handle stays on fp16x3
// c3_model.hip includes this file behind c3_mixed.h: its kernel is instantiated behind every other one (c3_forward.h says why).
#pragma once
#include "c3_forward.h"

constexpr int kCensusThreads = 256;
constexpr uint32_t kCensusInf = 0x7f800000u;

// census[c] = max(census[c], max over rows m of |x[m][c]|), x fp32 [M][C] with C = 64 << cshift.  A lane owns four channels (16 bytes, the
// C / 4 lanes of a row side by side) and every (256 / (C / 4))-th row of its workgroup's stride; the maximum is taken on the bit patterns
// of |x| -- non-negative floats order like unsigned integers, a NaN's pattern lies above infinity's and becomes it -- so it is exact and
// does not depend on the grid.  The lanes of a channel meet in LDS, then one atomic per channel and workgroup
__global__ void __launch_bounds__(kCensusThreads) channel_absmax_kernel(const float *__restrict__ x, uint32_t *__restrict__ census, int M, int cshift) {
    __shared__ uint32_t red[kCensusThreads * 4];
    const int tid = threadIdx.x, C = 64 << cshift;
    const int lanes_per_row = C >> 2, rows_per_pass = kCensusThreads / lanes_per_row;
    const int q = tid & (lanes_per_row - 1), r0 = tid >> (4 + cshift);
    uint32_t mx[4] = {0u, 0u, 0u, 0u};
    for (int64_t row = (int64_t)blockIdx.x * rows_per_pass + r0; row < M; row += (int64_t)gridDim.x * rows_per_pass) {
        const uint4 v = *reinterpret_cast<const uint4 *>(x + row * C + 4 * q);
        mx[0] = max(mx[0], v.x & 0x7fffffffu), mx[1] = max(mx[1], v.y & 0x7fffffffu);
        mx[2] = max(mx[2], v.z & 0x7fffffffu), mx[3] = max(mx[3], v.w & 0x7fffffffu);
    }
    for (int j = 0; j < 4; ++j) red[tid * 4 + j] = min(mx[j], kCensusInf);  // = red[r0 * C + 4 q + j]
    __syncthreads();
    if (tid < C) {
        uint32_t v = 0u;
        for (int r = 0; r < rows_per_pass; ++r) v = max(v, red[r * C + tid]);
        if (v) atomicMax(census + tid, v);
    }
}

// tap() of a census pass: the n windows of convolution `id` that the launch just enqueued on s wrote at src (fp32 NHWC)
static int census_tap(c3_model *m, hipStream_t s, int id, const float *src, int64_t n) {
    if (id >= 9) return 0;
    int hh[10], ww[10];
    fa_geometry(m, hh, ww);
    const int C = kConvCout[id], cshift = C == 64 ? 0 : C == 128 ? 1 : 2;
    const int64_t M = n * hh[id + 1] * ww[id + 1];
    if (M <= 0) return 0;
    if (M > INT32_MAX) return fail("internal: %lld rows in the census of layer %d", (long long)M, id);
    const int rows_per_pass = kCensusThreads / (C / 4);
    const int grid = (int)std::min<int64_t>((M + rows_per_pass - 1) / rows_per_pass, m->wg_slots);
    hipLaunchKernelGGL(channel_absmax_kernel, dim3((unsigned)grid), dim3(kCensusThreads), 0, s, src, m->census_dev + id * 256, (int)M, cshift);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the groups: stage0, inner0, stage1, inner1, stage2, inner2 (c3_pack.h FaChannelExps), 2 x (64 + 128 + 256) = kCalChannels entries ----
struct CalGroup { int at, n, layer[2]; };  // first entry, channels, the convolutions that write the group (-1: only one)
static CalGroup cal_group(int g) {
    static const int at[6] = {0, 64, 128, 256, 384, 640};
    const int s = g / 2;
    if (g % 2) return {at[g], kConvCout[3 * s], {3 * s + 1, -1}};
    return {at[g], kConvCout[3 * s], {3 * s, 3 * s + 2}};
}
static std::vector<int> *cal_group_exps(FaChannelExps &ex, int g) { return g % 2 ? &ex.inner[g / 2] : &ex.stage[g / 2]; }

// c3_model_load: the exponents of this load as fa_channel_exps gave them (k0) and as the handle runs them (k = k0 - lowering, not below the
// clamp fa_channel_exps has); ex leaves as k.  Without a lowering ex is untouched: the packed bytes are those of a handle that never heard of it
static int apply_channel_lowering(c3_model *m, FaChannelExps &ex) {
    for (int g = 0; g < 6; ++g) {
        const CalGroup G = cal_group(g);
        std::vector<int> &k = *cal_group_exps(ex, g);
        if ((int)k.size() != G.n) return fail("internal: channel group %d has %zu exponents", g, k.size());
        for (int c = 0; c < G.n; ++c) {
            m->chan_k0[G.at + c] = (int8_t)k[c];
            if (m->lowering_set) k[c] = std::max(-40, k[c] - (int)m->lowering[G.at + c]);
            m->chan_k[G.at + c] = (int8_t)k[c];
        }
    }
    m->chan_ok = true;
    return 0;
}

// The packing part of a full-alignment c3_model_load -- and ALL a repack of the range guard's recalibration runs (fa_repack below): the
// exponents of the checkpoint, the lowering in force, the nine convolutions, the FC tail
static int fa_pack_weights(c3_model *m, const TensorMap &tm) {
    int cin = m->C;
    if (3 * cin > 32) return fail("full-alignment input_channels %d not supported (3*C must be <= 32)", cin);
    FaChannelExps ex;
    TRY(fa_channel_exps(tm, ex));
    TRY(apply_channel_lowering(m, ex));  // (records k0; changes ex only while a lowering is set)
    for (int l = 0; l < 9; ++l) {
        TRY(pack_conv(m, tm, l, cin, ex));
        m->act_exp[l] = *ex.out_of(l);
        cin = kConvCout[l];
    }
    return pack_tail(m, tm, &ex.stage[2]);
}
// c3_model_load under the RECALIBRATE policy: the float32 tensors as given, for the repacks to come
static void keep_tensors(c3_model *m, const TensorMap &tm) {
    m->kept.clear();
    m->kept.reserve(tm.size());
    for (const auto &kv : tm) {
        size_t n = 1;
        for (int64_t d : kv.second.shape) n *= (size_t)d;
        m->kept.push_back(KeptTensor{kv.first, kv.second.shape, std::vector<float>(kv.second.d, kv.second.d + n)});
    }
}
// The weights packed again from the kept tensors with the lowering now in force: the bytes of c3_model_set_channel_lowering followed by
// c3_model_load, and nothing else a load does -- verify mode's totals, the precision plan, taps, a profile, the exact form's weights and
// what C3HIP_FP32 decided stay.  The caller has made sure that nothing runs on the weights
static int fa_repack(c3_model *m) {
    if (m->kept.empty()) return fail("internal: a repack without the tensors of the last load");
    TensorMap tm;
    for (const KeptTensor &t : m->kept) tm[t.name] = TensorView{t.data.data(), t.shape};
    TRY(fa_pack_weights(m, tm));
    m->layer_exp_ok = false;  // (layer records: the channel exponents changed)
    return 0;
}

// The rule for one group.  e[c]: binary exponent of the scaled maximum s[c] = f * 2^e[c], f in [0.5, 1) (frexp); live[c]: s[c] > 0
static void calibration_rule(const int *e, const uint8_t *live, int n, int cap_log2, uint8_t *lowering_out) {
    std::vector<int> d(n, 0), seen;
    for (int c = 0; c < n; ++c)
        if (live[c]) d[c] = std::max(0, e[c] - cap_log2), seen.push_back(d[c]);
    std::sort(seen.begin(), seen.end());
    const int d_group = seen.empty() ? 0 : seen[(seen.size() - 1) / 2];  // the lower median
    for (int c = 0; c < n; ++c) lowering_out[c] = (uint8_t)std::min(255, std::max(d[c], d_group));
}

// a pass's device census (the units of the current load) joins the handle's, in the checkpoint's units: exact, and it commutes with the maximum
static void census_merge(c3_model *m, const std::vector<float> &dev, int64_t batch) {
    for (int l = 0; l < 9; ++l)
        for (int c = 0; c < kConvCout[l]; ++c) m->census[l][c] = std::max(m->census[l][c], std::ldexp(dev[l * 256 + c], -m->act_exp[l][c]));
    m->census_windows += batch;
}
static int calibration_solve(c3_model *m, int cap_log2, uint8_t *lowering_out);
static int calibration_handle(c3_model *m, const char *who) {
    if (!m) return fail("null model");
    if (m->kind != C3_KIND_FULL_ALIGNMENT)
        return fail("%s: calibration is for full-alignment handles (the gates of the pileup network's LSTMs are not homogeneous: a channel cannot be rescaled)", who);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    return 0;
}

extern "C" {

int c3_calibration_rule(const float *scaled_max, int n, int cap_log2, uint8_t *lowering_out) {
    if (!scaled_max || !lowering_out) return fail("null argument");
    if (n < 1) return fail("c3_calibration_rule: a group has at least one channel, got %d", n);
    if (cap_log2 < 4 || cap_log2 > 13) return fail("cap_log2 must be in [4, 13], got %d", cap_log2);
    std::vector<int> e(n, 0);
    std::vector<uint8_t> live(n, 0);
    for (int c = 0; c < n; ++c) {
        if (!std::isfinite(scaled_max[c])) return fail("c3_calibration_rule: the maximum of channel %d is not finite", c);
        if (scaled_max[c] < 0.f) return fail("c3_calibration_rule: the maximum of channel %d is negative", c);
        if ((live[c] = scaled_max[c] > 0.f)) (void)std::frexp(scaled_max[c], &e[c]);
    }
    calibration_rule(e.data(), live.data(), n, cap_log2, lowering_out);
    return 0;
}

int c3_model_calibrate_reset(c3_model *m) {
    TRY(calibration_handle(m, "c3_model_calibrate_reset"));
    memset(m->census, 0, sizeof(m->census));
    m->census_windows = 0;
    return 0;
}

int c3_model_calibrate(c3_model *m, const void *x_host, int x_dtype, int64_t batch, float *y_host) {
    TRY(calibration_handle(m, "c3_model_calibrate"));
    if (!m->loaded) return fail("model has no weights: call c3_model_load first");
    if (batch < 0) return fail("negative batch");
    if (batch > 0 && !x_host) return fail("null buffer");
    if (x_dtype != C3_DTYPE_I8) return fail("full-alignment windows must be int8 (got dtype %d)", x_dtype);
    if (batch == 0) return 0;
    HIP_TRY(hipSetDevice(m->device));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    if (!m->census_dev) HIP_TRY(hipMalloc((void **)&m->census_dev, 9 * 256 * sizeof(uint32_t)));
    const int64_t wbytes = c3_model_window_bytes(m, x_dtype), piece = max_microbatch(m);
    void *x_dev = nullptr;
    float *y_dev = nullptr;
    const int64_t cap = std::min(batch, piece);
    int rc = 0;
    if (hipMalloc(&x_dev, (size_t)(cap * wbytes)) != hipSuccess || hipMalloc((void **)&y_dev, (size_t)(cap * m->row) * sizeof(float)) != hipSuccess)
        (void)hipGetLastError(), rc = fail("c3_model_calibrate: no device memory for %lld windows", (long long)cap);
    if (rc == 0 && hipMemsetAsync(m->census_dev, 0, 9 * 256 * sizeof(uint32_t), s) != hipSuccess) rc = fail("c3_model_calibrate: hipMemsetAsync failed");
    // the fp32 forms for this call alone: what the handle runs, reports and taps stays as it is (c3_hostring.h shadow_pass does the same)
    const c3_model::Choices reported = m->choice;
    const bool f16 = m->f16_ok, tap_call = m->tap_call, prof = m->prof;  // (prof: the pass adds no records to a profile that is being taken)
    const int64_t tap_base = m->tap_base;
    for (int64_t off = 0; off < batch && rc == 0; off += piece) {
        const int64_t n = std::min(piece, batch - off);
        rc = h2d_staged(x_dev, (const char *)x_host + off * wbytes, (size_t)(n * wbytes), s);
        if (rc) break;
        m->f16_ok = false, m->census_pass = 1, m->tap_call = true, m->prof = false;  // (tap_call: forward_device leaves the tap buffers of the last call alone)
        rc = forward_device(m, s, x_dev, x_dtype, n, y_dev);
        m->f16_ok = f16, m->census_pass = 0, m->tap_call = tap_call, m->prof = prof, m->tap_base = tap_base, m->choice = reported;
        if (rc) break;
        if (y_host) rc = d2h_staged(y_host + off * m->row, y_dev, (size_t)(n * m->row) * sizeof(float), s);
        else if (hipStreamSynchronize(s) != hipSuccess) rc = fail("c3_model_calibrate: hipStreamSynchronize failed");
    }
    // the device values carry the exponents of this load; the census is kept in the checkpoint's units (exact, and it commutes with the maximum)
    std::vector<float> dev(9 * 256, 0.f);
    if (rc == 0) rc = d2h_staged(dev.data(), m->census_dev, dev.size() * sizeof(float), s);
    if (rc == 0 && hipStreamSynchronize(s) != hipSuccess) rc = fail("c3_model_calibrate: hipStreamSynchronize failed");
    const std::string why = g_err;
    (void)hipDeviceSynchronize();
    if (x_dev) (void)hipFree(x_dev);
    if (y_dev) (void)hipFree(y_dev);
    if (rc) return g_err = why, rc;
    census_merge(m, dev, batch);
    return 0;
}

int c3_model_calibration_census(c3_model *m, float *absmax_out, int64_t *windows_out) {
    TRY(calibration_handle(m, "c3_model_calibration_census"));
    if (absmax_out) memcpy(absmax_out, m->census, sizeof(m->census));
    if (windows_out) *windows_out = m->census_windows;
    return 0;
}

int c3_model_calibration_solve(c3_model *m, int cap_log2, uint8_t *lowering_out) {
    TRY(calibration_handle(m, "c3_model_calibration_solve"));
    return calibration_solve(m, cap_log2, lowering_out);
}

}  // extern "C"

// (the range guard's recalibration solves inside c3_predict_wait, with other slots of the ring still waiting to be read)
static int calibration_solve(c3_model *m, int cap_log2, uint8_t *lowering_out) {
    if (!lowering_out) return fail("null argument");
    if (cap_log2 < 4 || cap_log2 > 13) return fail("cap_log2 must be in [4, 13], got %d", cap_log2);
    if (!m->loaded || !m->chan_ok) return fail("model has no weights: call c3_model_load first");
    if (m->census_windows <= 0) return fail("c3_model_calibration_solve: no census yet: call c3_model_calibrate first");
    for (int l = 0; l < 9; ++l)
        for (int c = 0; c < kConvCout[l]; ++c)
            if (!std::isfinite(m->census[l][c]))
                return fail("c3_model_calibration_solve: the census of layer %d (%s), channel %d is not finite", l, kFaLayers[l].name, c);
    for (int g = 0; g < 6; ++g) {
        const CalGroup G = cal_group(g);
        std::vector<int> e(G.n, 0);
        std::vector<uint8_t> live(G.n, 0);
        for (int c = 0; c < G.n; ++c) {
            // s = A * 2^k0 through its exponent: the same number whatever the float range
            const float a = std::max(m->census[G.layer[0]][c], G.layer[1] >= 0 ? m->census[G.layer[1]][c] : 0.f);
            if ((live[c] = a > 0.f)) (void)std::frexp(a, &e[c]), e[c] += m->chan_k0[G.at + c];
        }
        calibration_rule(e.data(), live.data(), G.n, cap_log2, lowering_out + G.at);
        for (int c = 0; c < G.n; ++c)  // k0 - lowering stays at or above the clamp of fa_channel_exps
            lowering_out[G.at + c] = (uint8_t)std::min<int>(lowering_out[G.at + c], m->chan_k0[G.at + c] + 40);
    }
    m->solved = true, m->solved_cap = cap_log2, m->solved_windows = m->census_windows;
    memcpy(m->solved_lowering, lowering_out, kCalChannels);
    return 0;
}

extern "C" {

int c3_model_set_channel_lowering(c3_model *m, const uint8_t *lowering) {
    TRY(calibration_handle(m, "c3_model_set_channel_lowering"));
    m->lowering_set = lowering != nullptr;
    if (lowering) memcpy(m->lowering, lowering, kCalChannels);
    else memset(m->lowering, 0, kCalChannels);
    // its origin travels with it: the handle's own last solve where this is its result, else not known until the caller says
    const bool own = lowering && m->solved && !memcmp(lowering, m->solved_lowering, kCalChannels);
    m->lowering_cap = own ? m->solved_cap : 0, m->lowering_windows = own ? m->solved_windows : 0;
    return 0;
}

int c3_model_set_calibration_origin(c3_model *m, int cap_log2, int64_t windows) {
    TRY(calibration_handle(m, "c3_model_set_calibration_origin"));
    if (!m->lowering_set) return fail("c3_model_set_calibration_origin: no lowering is set");
    if (cap_log2 < 0 || cap_log2 > 13 || windows < 0) return fail("c3_model_set_calibration_origin: cap_log2 in [0, 13] and windows >= 0 expected, got %d and %lld", cap_log2, (long long)windows);
    m->lowering_cap = cap_log2, m->lowering_windows = windows;
    return 0;
}

int c3_model_channel_exps(c3_model *m, int8_t *k0_out, int8_t *k_out) {
    TRY(calibration_handle(m, "c3_model_channel_exps"));
    if (!m->loaded || !m->chan_ok) return fail("model has no weights: call c3_model_load first");
    if (k0_out) memcpy(k0_out, m->chan_k0, kCalChannels);
    if (k_out) memcpy(k_out, m->chan_k, kCalChannels);
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the range guard's recalibration
// The policy C3_RANGE_RECALIBRATE (include/c3hip.h c3_model_set_range_policy).  The sticky guard answers a trip with an fp32 pass over the
// windows that tripped it; that pass is the best sample there is, so here it also takes the census, the rule runs on it, the weights are
// packed again with the new lowering and the handle stays on the fp16x3 kernels.  No kernel of its own: the fp32 forms, the census kernel
// and the load's packing as they are.
static int parse_range_policy(const char *text, int *policy, int *max_recal, const char *what) {
    static const char *const expected = "expected sticky, recalibrate or recalibrate:<n> with n >= 0";
    if (!text) return fail("%s: null text (%s)", what, expected);
    if (!strcmp(text, "sticky")) return *policy = C3_RANGE_STICKY, *max_recal = 0, 0;
    if (!strcmp(text, "recalibrate")) return *policy = C3_RANGE_RECALIBRATE, *max_recal = 4, 0;
    if (!strncmp(text, "recalibrate:", 12)) {
        const char *p = text + 12;
        long n = 0;
        int digits = 0;
        for (; *p >= '0' && *p <= '9' && digits < 7; ++p, ++digits) n = 10 * n + (*p - '0');
        if (digits > 0 && !*p) return *policy = C3_RANGE_RECALIBRATE, *max_recal = (int)n, 0;
    }
    return fail("%s=%s: %s", what, text, expected);
}

// what the sticky guard prints, and why this handle is back on its behaviour
static void range_guard_fall_back(c3_model *m, const char *why) {
    fprintf(stderr, "libc3hip: activations beyond the range of the fp16x3 kernels; this handle continues on fp32 matrix instructions (range guard: %s)\n", why);
    m->f16_ok = false, m->precision = "fp32-range-guard";
    m->rstats.fell_back = 1;
    snprintf(m->rstats.reason, sizeof(m->rstats.reason), "%s", why);
}

extern "C" {  // (declared in c3_hostring.h beside range_guard_rerun, inside its extern "C" block)

// A trip under the policy (c3_hostring.h c3_predict_wait, c3_model.hip c3_predict_device_checked; the arguments of range_guard_rerun, the
// batch's lane active).  On return y_dev holds the rows of the fp32 forms -- bit for bit the sticky guard's -- and the handle either runs the
// fp16x3 kernels on weights packed with the new lowering or has fallen back to the sticky behaviour
static int range_guard_recalibrate(c3_model *m, hipStream_t s, const void *x_dev, int x_dtype, int64_t batch, float *y_dev, int64_t tap_off,
                                   const int32_t *starts, const int32_t *depth, const ExpandEntry *rows) {
    ++m->rstats.trips;
    // nothing may run on the weights while they are packed again: every lane's work, the transfers included.  The rows and flag copies of the
    // other slots in flight have landed in their pinned buffers by then; their own c3_predict_wait deals with them
    for (const Lane &L : m->lanes)
        if (L.stream) HIP_TRY(hipStreamSynchronize(L.stream));
    if (m->h2d_stream) HIP_TRY(hipStreamSynchronize(m->h2d_stream));
    if (m->rstats.recalibrations >= m->range_max_recal) {
        range_guard_fall_back(m, "allowance of recalibrations used up");
        return range_guard_rerun(m, s, x_dev, x_dtype, batch, y_dev, tap_off, starts, depth, rows);
    }
    // the fp32 pass of range_guard_rerun, with the census behind every convolution (census_pass 2: a user's taps are served as well)
    if (!m->census_dev) HIP_TRY(hipMalloc((void **)&m->census_dev, 9 * 256 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(m->census_dev, 0, 9 * 256 * sizeof(uint32_t), s));
    const c3_model::Choices reported = m->choice;
    m->f16_ok = false, m->census_pass = 2, m->tap_call_off = tap_off;
    int rc = forward_device(m, s, x_dev, x_dtype, batch, y_dev, starts, depth, rows);
    m->f16_ok = true, m->census_pass = 0, m->tap_call_off = 0;
    TRY(rc);
    std::vector<float> dev(9 * 256, 0.f);
    TRY(d2h_staged(dev.data(), m->census_dev, dev.size() * sizeof(float), s));
    HIP_TRY(hipStreamSynchronize(s));
    census_merge(m, dev, batch);  // (in the units of the packing that just ran)
    bool finite = true;
    for (int l = 0; l < 9; ++l)
        for (int c = 0; c < kConvCout[l]; ++c) finite &= std::isfinite(m->census[l][c]);
    if (!finite) return range_guard_fall_back(m, "census not finite"), 0;
    // the rule at the cap of the lowering in force, else 2^10; never up
    const int cap = m->lowering_set && m->lowering_cap >= 4 && m->lowering_cap <= 13 ? m->lowering_cap : 10;
    uint8_t solved[kCalChannels];
    TRY(calibration_solve(m, cap, solved));
    int moved = 0;
    for (int c = 0; c < kCalChannels; ++c) {
        const uint8_t old = m->lowering_set ? m->lowering[c] : 0;
        solved[c] = std::max(solved[c], old), moved += solved[c] != old;
    }
    if (!moved) return range_guard_fall_back(m, "the census asks for no further lowering"), 0;
    memcpy(m->lowering, solved, kCalChannels);
    m->lowering_set = true, m->lowering_cap = cap, m->lowering_windows = m->census_windows;
    if (fa_repack(m) != 0) {  // (half-packed weights answer nothing)
        m->loaded = false;
        return 1;
    }
    HIP_TRY(hipMemsetAsync(m->range_flag, 0, 256, s));
    HIP_TRY(hipStreamSynchronize(s));
    m->choice = reported;  // what c3_model_describe says of the last pass stays the product pass's: that is what the handle runs
    ++m->pack_epoch, ++m->rstats.recalibrations;
    m->rstats.channels_lowered = moved, m->rstats.cap_log2 = cap;
    fprintf(stderr, "libc3hip: activations beyond the range of the fp16x3 kernels; recalibrated from this batch (%d channels lowered, census of %lld "
                    "windows); this handle stays on the fp16x3 kernels\n", moved, (long long)m->census_windows);
    return 0;
}

int c3_range_policy_check(const char *text) {
    int policy = 0, max_recal = 0;
    return parse_range_policy(text, &policy, &max_recal, "c3_range_policy_check");
}

int c3_model_set_range_policy(c3_model *m, int policy, int max_recalibrations) {
    if (!m) return fail("null model");
    if (policy != C3_RANGE_STICKY && policy != C3_RANGE_RECALIBRATE) return fail("c3_model_set_range_policy: unknown policy %d", policy);
    if (max_recalibrations < 0) return fail("c3_model_set_range_policy: max_recalibrations must be >= 0, got %d", max_recalibrations);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    if (policy == C3_RANGE_RECALIBRATE) {
        if (m->kind != C3_KIND_FULL_ALIGNMENT)
            return fail("c3_model_set_range_policy: recalibration is for full-alignment handles (the pileup network's LSTM layers have no ReLU "
                        "homogeneity to rescale a channel through)");
        if (m->loaded && m->kept.empty())
            return fail("c3_model_set_range_policy: this handle holds no copy of the tensors it was loaded from: set it before c3_model_load");
    }
    m->range_policy = policy, m->range_max_recal = policy == C3_RANGE_RECALIBRATE ? max_recalibrations : 0;
    if (policy == C3_RANGE_STICKY) std::vector<KeptTensor>().swap(m->kept);
    return 0;
}

int c3_model_range_stats(c3_model *m, c3_range_stats *out) {
    if (!m) return fail("null model");
    if (!out) return fail("null argument");
    *out = m->rstats;
    out->census_windows = m->census_windows, out->policy = m->range_policy, out->max_recalibrations = m->range_max_recal;
    return 0;
}

}  // extern "C"
