// c3_model.hip -- the C ABI of include/c3hip.h: model handles (create / geometry / load / destroy), the device-resident entry
// points and their range guard.  The units it is made of are listed in c3_model.h.
#include "c3_model.h"
#include "c3_pack.h"
#include "c3_forward.h"
#include "c3_hostring.h"
#include "c3_comm.h"
#include "c3_debug.h"
#include "c3_rows.h"
#include "c3_mixed.h"  // (behind every kernel of the handle without a plan: c3_forward.h says why)
#include "c3_calibrate.h"  // (last, for the same reason)
#include "c3_exact.h"  // (behind every other kernel: the exact form is an instrument and moves none of them)
#include "c3_variants.h"  // (host code only: what the three modes below share)
#include "c3_jackknife.h"  // (jackknife mode: its kernels sit in a section of their own behind `.c3_refine_text`)
#include "c3_subsample.h"  // (subsample mode: its kernels sit in a section of their own behind `.c3_jackknife_text`)
#include "c3_occlude.h"  // (occlusion mode: its kernels sit in a section of their own behind `.c3_subsample_text`)
#include "c3_gvcf.h"  // (gVCF mode: no model; its kernels sit in a section of their own behind `.c3_occlude_text`)
#include "c3_pileup.h"  // (pileup from reads: no model; its kernels sit in a section of their own behind `.c3_gvcf_text`)
#include "c3_fa_reads.h"  // (full alignment from reads: its kernels sit in a section of their own behind `.c3_pileup_text`)
#include "c3_hap_reads.h"  // (haplotagging the reads: its kernels sit in a section of their own behind `.c3_fa_text`)
#include "c3_dwell.h"  // (the dwell channel of those windows: its kernels sit in a section of their own behind `.c3_hap_text`)

extern "C" {

const char *c3_version(void) { return "c3hip 0.5.6 (gfx950, fp32 data, fp16x3 split matrix products) srchash:" C3HIP_SRC_HASH; }
const char *c3_last_error(void) { return g_err.c_str(); }

int c3_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) return 0;
    if (e != hipSuccess) {
        fail("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return -1;
    }
    return n;
}

int c3_mem_info(int device, size_t *free_bytes, size_t *total_bytes) {
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(device));
    size_t f = 0, t = 0;
    hipError_t e = hipMemGetInfo(&f, &t);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail("hipMemGetInfo failed: %s", hipGetErrorString(e));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}

int c3_device_pci_bus_id(int device, char *buf, int buf_bytes) {
    if (!buf || buf_bytes < 16) return fail("c3_device_pci_bus_id: buffer of at least 16 bytes needed");
    HIP_TRY(hipDeviceGetPCIBusId(buf, buf_bytes, device));
    for (char *c = buf; *c; ++c) *c = (char)tolower((unsigned char)*c);  // sysfs spells the address in lower case
    return 0;
}

}  // extern "C"

// ---- the per-layer precision plan (c3_model.h layer_f16): "lstm2,l4" -> mask.  Plain host code; `what` names the source in the error
static int parse_layer_names(int kind, const char *names, uint32_t *mask, const char *what) {
    const LayerName *mine, *other;
    const int n_mine = layer_names(kind, &mine);
    if (!n_mine) return fail("%s: unknown model kind %d", what, kind);
    if (!names) return fail("%s: null layer names", what);
    const int other_kind = kind == C3_KIND_PILEUP ? C3_KIND_FULL_ALIGNMENT : C3_KIND_PILEUP;
    const int n_other = layer_names(other_kind, &other);
    const std::string valid = layer_mask_text(kind, layer_mask_all(kind));
    uint32_t out = 0;
    if (!strcmp(names, "all")) return *mask = layer_mask_all(kind), 0;
    for (const char *p = names; *p;) {
        const char *e = strchr(p, ',');
        const std::string entry = e ? std::string(p, e) : std::string(p);
        if (entry.empty()) return fail("%s: empty entry in \"%s\" (expected names out of %s, \"all\" or \"\")", what, names, valid.c_str());
        uint32_t bit = 0;
        for (int i = 0; i < n_mine; ++i)
            if (entry == mine[i].name) bit = mine[i].bit;
        if (!bit) {
            for (int i = 0; i < n_other; ++i)
                if (entry == other[i].name)
                    return fail("%s: \"%s\" is a layer of the %s network; this one has %s", what, entry.c_str(),
                                other_kind == C3_KIND_PILEUP ? "pileup" : "full-alignment", valid.c_str());
            return fail("%s: unknown layer \"%s\" (expected names out of %s, \"all\" or \"\")", what, entry.c_str(), valid.c_str());
        }
        out |= bit;
        if (!e) break;
        p = e + 1;
        if (!*p) return fail("%s: empty entry in \"%s\" (expected names out of %s, \"all\" or \"\")", what, names, valid.c_str());
    }
    *mask = out;
    return 0;
}

extern "C" {

int c3_layer_precision_check(int kind, const char *names) {
    uint32_t mask = 0;
    return parse_layer_names(kind, names, &mask, "c3_layer_precision_check");
}

int c3_model_set_layer_precision(c3_model *m, const char *names) {
    if (!m) return fail("null model");
    uint32_t mask = 0;
    TRY(parse_layer_names(m->kind, names, &mask, "c3_model_set_layer_precision"));
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    m->fp32_plan = mask;
    return 0;
}

int c3_model_layer_precision(c3_model *m, char *buf, int buf_bytes) {
    if (!m || !buf || buf_bytes <= 0) return fail("null argument");
    const std::string text = layer_mask_text(m->kind, m->fp32_plan | m->fp32_auto);
    if ((int)text.size() >= buf_bytes) return fail("c3_model_layer_precision: buffer of %d bytes needed", (int)text.size() + 1);
    memcpy(buf, text.c_str(), text.size() + 1);
    return 0;
}

c3_model *c3_model_create(int kind, int in_channels, int add_indel_length, int device) {
    if (kind != C3_KIND_PILEUP && kind != C3_KIND_FULL_ALIGNMENT) {
        fail("unknown model kind %d", kind);
        return nullptr;
    }
    if (kind == C3_KIND_PILEUP && (in_channels < 1 || in_channels > 4 * kFusedKS)) {
        fail("pileup input_channels must be in [1,%d], got %d", 4 * kFusedKS, in_channels);
        return nullptr;
    }
    if (kind == C3_KIND_FULL_ALIGNMENT && (in_channels < 1 || in_channels > 10)) {
        fail("full-alignment input_channels must be in [1,10], got %d", in_channels);
        return nullptr;
    }
    int ndev = c3_device_count();
    if (ndev <= 0) {
        fail("no HIP device visible (libc3hip has no CPU fallback)");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail("device %d out of range (%d visible)", device, ndev);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        fail("hipSetDevice(%d) failed", device);
        return nullptr;
    }
    c3_model *m = new c3_model();
    m->kind = kind, m->C = in_channels, m->add_indel = add_indel_length ? 1 : 0, m->device = device;
    if (hipMalloc((void **)&m->range_flag, 256) != hipSuccess || hipMemset(m->range_flag, 0, 256) != hipSuccess) {
        fail("c3_model_create: cannot allocate the range flag");
        delete m;
        return nullptr;
    }
    m->nb = m->add_indel ? 4 : 2, m->nout = m->add_indel ? 90 : 24;
    m->row = m->nout;
    m->FC = kind == C3_KIND_PILEUP ? 128 : 256;
    m->K4 = kind == C3_KIND_PILEUP ? m->positions * 320 : 14 * 256;
    if (hipStreamCreateWithFlags(&m->lanes[0].stream, hipStreamNonBlocking) != hipSuccess) {  // (a further lane's: use_lane; the transfer stream: c3_hostring.h)
        fail("hipStreamCreate failed");
        delete m;
        return nullptr;
    }
    if (getenv("C3HIP_KEEP_ACTIVATIONS")) m->keep = true;
    if (const char *e = getenv("C3HIP_FP32")) {  // an explicit choice: 1 = start on the fp32-MFMA forms (what the range guard falls back to), 0 = fp16x3, no automatism
        m->f16_ok = m->forced_f16 = atoi(e) == 0, m->precision_forced = true;
        if (!m->f16_ok) m->precision = "fp32-forced";
    }
    if (const char *e = getenv("C3HIP_AUTO_FP32")) m->auto_fp32_at = (float)atof(e);
    // the per-layer plan (c3_model.h): an invalid value fails the creation -- a precision request is never dropped silently
    if (const char *e = getenv("C3HIP_FP32_LAYERS")) {
        if (parse_layer_names(kind, e, &m->fp32_plan, "C3HIP_FP32_LAYERS")) {
            c3_model_destroy(m);
            return nullptr;
        }
    }
    if (const char *e = getenv("C3HIP_AUTO_FP32_LAYERS")) {  // what the load-time rule escalates instead of the whole handle
        if (parse_layer_names(kind, e, &m->auto_layers, "C3HIP_AUTO_FP32_LAYERS")) {
            c3_model_destroy(m);
            return nullptr;
        }
    }
    if (const char *e = getenv("C3HIP_CONV1_FUSED")) m->conv1_fused = atoi(e) != 0;
    if (const char *e = getenv("C3HIP_WINO")) m->wino = atoi(e);
    if (const char *e = getenv("C3HIP_SPP_FUSED")) m->spp_fused = atoi(e) != 0;
    m->tail_fused = kind == C3_KIND_PILEUP;  // (profiles/r04_e_ab_tail_pileup.txt, r04_e_ab_tail_fa.txt)
    if (const char *e = getenv("C3HIP_FA_TAIL")) {  // a form switch (c3_model.h fa_tail); a value that names no form fails the creation
        static const struct { const char *name; int v; } forms[] = {{"auto", 0}, {"split", -1}, {"w4", 4}, {"w8", 8}, {"w16", 16}};
        const auto *f = std::find_if(std::begin(forms), std::end(forms), [e](const auto &x) { return !strcmp(x.name, e); });
        if (f == std::end(forms)) {
            fail("C3HIP_FA_TAIL=%s: expected auto, split, w4, w8 or w16", e);
            c3_model_destroy(m);
            return nullptr;
        }
        m->fa_tail = f->v;
    }
    if (const char *e = getenv("C3HIP_WAVE_PRIO")) m->wave_prio = atoi(e) != 0;  // (c3_model.h wave_prio)
    if (const char *e = getenv("C3HIP_RANGE_GUARD")) {  // the range-guard policy a full-alignment handle starts with; a value that names none fails the creation
        int policy = 0, max_recal = 0;
        if (parse_range_policy(e, &policy, &max_recal, "C3HIP_RANGE_GUARD")) {
            c3_model_destroy(m);
            return nullptr;
        }
        if (kind == C3_KIND_FULL_ALIGNMENT) m->range_policy = policy, m->range_max_recal = max_recal;
    }
    if (const char *e = getenv("C3HIP_HALF_TILES")) m->half_tiles = atoi(e) != 0;
    if (const char *e = getenv("C3HIP_PACK_ROWS")) m->pack_rows = kind == C3_KIND_FULL_ALIGNMENT && atoi(e) != 0;  // (c3_expand.h; default off)
    // two lanes for the ring (c3_model.h Lane): the kind's default follows the same-box A/B of profiles/r06_i_ab_ring_lanes.txt
    // (one MI355X, alternating: full alignment ring 728 - 732 k -> 768 - 775 k windows/s at B = 256 but 807 - 809 k -> 768 - 778 k at B = 1000; pileup
    // 4.24 M -> 4.32 - 4.33 M at B = 1024): more than one lane, for batches that do not fill the chip by themselves
    // ... and three against two lanes (run 11, another box): full alignment ring 703 - 704 k (one lane) -> 745 k (two) -> 769 - 770 k (three) at B = 256;
    // pileup 4.11 - 4.14 M -> 4.23 - 4.26 M (two) -> 4.07 - 4.08 M (three: three recurrences side by side starve each other)
    m->ring_lanes = kind == C3_KIND_FULL_ALIGNMENT ? 3 : 2;
    m->lane_max_batch = kind == C3_KIND_FULL_ALIGNMENT ? 512 : 1024;
    if (const char *e = getenv("C3HIP_RING_LANES")) m->ring_lanes = std::min(std::max(atoi(e), 1), kMaxLanes);
    if (const char *e = getenv("C3HIP_RING_LANES_MAX_BATCH")) m->lane_max_batch = atoll(e);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            m->wg_slots = 2 * prop.multiProcessorCount;
    }
    if (hipMalloc((void **)&m->zeros, 256) != hipSuccess || hipMemset(m->zeros, 0, 256) != hipSuccess) {
        fail("hipMalloc(zero page) failed");
        c3_model_destroy(m);
        return nullptr;
    }
    return m;
}

int c3_model_set_geometry(c3_model *m, int depth, int positions) {
    if (!m) return fail("null model");
    if (positions < 1 || depth < 1) return fail("bad geometry %dx%d", depth, positions);
    if (depth == m->depth && positions == m->positions) return 0;  // (nothing changes: the workspaces and the weights stay)
    // refused before anything is touched: the workspaces freed below are what a batch in flight computes in, and c3_predict_wait
    // reads the handle's geometry and weights when the range guard runs a batch again
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    const int K4 = m->kind == C3_KIND_PILEUP ? positions * 320 : m->K4;
    if (K4 % kBK) return fail("unsupported geometry: L4 fan-in %d is not a multiple of %d", K4, kBK);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    m->depth = depth, m->positions = positions, m->K4 = K4;
    free_all_workspaces(m);
    exact_free_workspace(m);
    m->loaded = false;
    return 0;
}

int c3_model_output_size(const c3_model *m) { return m ? m->nout : -1; }
int c3_model_row_size(const c3_model *m) { return m ? m->row : -1; }

int c3_model_set_decode_columns(c3_model *m, int enable) {
    if (!m) return fail("null model");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    m->row = m->nout + (enable ? kDecodeCols : 0);
    return 0;
}

int64_t c3_model_window_bytes(const c3_model *m, int x_dtype) {
    if (!m) return -1;
    const int64_t item = x_dtype == C3_DTYPE_I32 ? 4 : 1;
    if (m->kind == C3_KIND_PILEUP) return item * m->positions * m->C;
    return item * m->depth * m->positions * m->C;
}

int c3_model_load(c3_model *m, const c3_tensor_desc *tensors, int n_tensors) {
    if (!m || (!tensors && n_tensors)) return fail("null argument");
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("a prediction is in flight: call c3_predict_wait first");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());  // (the device-resident entries may still run the weights before on a caller's stream)
    m->kept.clear();  // (the range-guard policy: the tensors of the load before; kept again at the end of a load that succeeds)
    TensorMap tm;
    for (int i = 0; i < n_tensors; ++i) {
        const c3_tensor_desc &t = tensors[i];
        if (!t.name) return fail("tensor %d has no name", i);
        const std::string name = t.name;
        const bool nbt = name.size() > 19 && name.compare(name.size() - 19, 19, "num_batches_tracked") == 0;
        if (nbt) continue;  // BatchNorm bookkeeping, unused in eval()
        if (t.dtype != C3_DTYPE_F32) return fail("tensor %s: only float32 parameters are supported", t.name);
        if (t.ndim < 1 || t.ndim > 4 || !t.data) return fail("tensor %s: bad descriptor", t.name);
        TensorView v;
        v.d = (const float *)t.data;
        v.shape.assign(t.shape, t.shape + t.ndim);
        tm[name] = v;
    }
    size_t expected = 0;
    if (m->kind == C3_KIND_PILEUP) {
        m->lstm_wmax = m->lstm_hh_norm = 0.f;
        TRY(pack_lstm(m, tm, 0, 128, m->C, 32));
        TRY(pack_lstm(m, tm, 1, 160, 256, 256));
        expected = 16;
        // precision escalation without a user switch (c3_model.h): decided once per load, from the weights alone
        if (!m->precision_forced) {
            const bool up = m->auto_fp32_at > 0.f && m->lstm_wmax >= m->auto_fp32_at;
            // C3HIP_AUTO_FP32_LAYERS: the rule escalates those layers and the handle stays on fp16x3 beside them
            const bool part = up && m->auto_layers && m->auto_layers != layer_mask_all(m->kind);
            m->fp32_auto = part ? m->auto_layers : 0;
            if (part) {
                m->precision_text = "fp32-auto(" + layer_mask_text(m->kind, m->fp32_auto) + ")";
                fprintf(stderr, "libc3hip: LSTM weights reach |w| = %.3g (>= %.3g): this pileup handle runs %s on the fp32 matrix instructions "
                                "(C3HIP_AUTO_FP32_LAYERS; C3HIP_FP32=0 keeps the fp16x3 kernels)\n", (double)m->lstm_wmax, (double)m->auto_fp32_at,
                        layer_mask_text(m->kind, m->fp32_auto).c_str());
                m->f16_ok = true, m->precision = m->precision_text.c_str();
            } else {
                if (up)
                    fprintf(stderr, "libc3hip: LSTM weights reach |w| = %.3g (>= %.3g): this pileup handle runs on the fp32 matrix instructions "
                                    "(C3HIP_FP32=0 keeps the fp16x3 kernels)\n", (double)m->lstm_wmax, (double)m->auto_fp32_at);
                m->f16_ok = !up, m->precision = up ? "fp32-auto" : "fp16x3";
            }
        }
    } else {
        TRY(fa_pack_weights(m, tm));  // (c3_calibrate.h: what a repack of the range guard's recalibration runs as well)
        expected = 54;
    }
    if (m->kind == C3_KIND_PILEUP) TRY(pack_tail(m, tm));
    expected += 2 + 4 * (size_t)m->nb;
    if (tm.size() != expected) {
        // strict like load_state_dict: report the first unexpected key
        return fail("Unexpected key(s) in state_dict: %zu tensors given, %zu expected", tm.size(), expected);
    }
    exact_free_weights(m);  // the exact form (c3_exact.h): the double weights travel with a load only while c3_model_set_exact is on
    if (m->exact.want) TRY(pack_exact(m, tm));
    // new weights, new start: what the range guard decided (f16_ok and the sticky device flag) was about the weights before.  The
    // handle goes back to what C3HIP_FP32 chose, else to the load-time decision above (pileup) or to fp16x3 (full alignment).
    if (m->precision_forced) m->f16_ok = m->forced_f16, m->precision = m->forced_f16 ? "fp16x3" : "fp32-forced";
    else if (m->kind == C3_KIND_FULL_ALIGNMENT) m->f16_ok = true, m->precision = "fp16x3";
    HIP_TRY(hipMemset(m->range_flag, 0, 256));
    HIP_TRY(hipDeviceSynchronize());  // (the handle's streams are non-blocking: the flag is zero before any of them runs again)
    verify_zero(m);  // verify mode: the totals were about the weights before; the setting stays
    refine_zero(m);  // refine mode: likewise
    m->layer_exp_ok = false;  // (layer records: the channel exponents are these weights')
    // the range-guard policy (c3_calibrate.h): the setting stays, the totals start again, and under RECALIBRATE the tensors are kept for its repacks
    m->rstats = c3_range_stats{}, m->pack_epoch = 0;
    if (m->range_policy == C3_RANGE_RECALIBRATE) keep_tensors(m, tm);
    m->loaded = true;
    return 0;
}

int c3_predict_device(c3_model *m, const void *x_dev, int x_dtype, int64_t batch, float *y_dev, void *stream) {
    if (!m) return fail("null model");
    if (batch > 0 && (!x_dev || !y_dev)) return fail("null buffer");
    HIP_TRY(hipSetDevice(m->device));
    // NULL is the HIP null stream itself (what torch's default stream is): work queued there is ordered with the
    // caller's other default-stream work.  Mapping NULL to the model's private non-blocking stream would let a
    // following torch op (y.cpu(), an RCCL gather) overtake the kernels.
    TRY(use_lane(m, 0));  // (calls on one handle must not overlap: the device-resident entries always work in the first lane)
    return forward_device(m, (hipStream_t)stream, x_dev, x_dtype, batch, y_dev);
}

int c3_predict_device_checked(c3_model *m, const void *x_dev, int x_dtype, int64_t batch, float *y_dev, void *stream) {
    if (!m) return fail("null model");
    if (batch > 0 && (!x_dev || !y_dev)) return fail("null buffer");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const bool f16 = m->f16_ok;
    TRY(use_lane(m, 0));
    TRY(forward_device(m, s, x_dev, x_dtype, batch, y_dev));
    if (!f16 || batch == 0) return 0;
    if (!m->pin_flag) {
        HIP_TRY(hipHostMalloc((void **)&m->pin_flag, 4096, hipHostMallocDefault));  // (a whole page: MADV_DONTFORK works on pages)
        keep_out_of_children(m->pin_flag, 4096);
    }
    const int64_t nf = batch * m->row;
    hipLaunchKernelGGL(rows_finite_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, y_dev, nf, m->range_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(m->pin_flag, m->range_flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*m->pin_flag) {
        TRY((range_recalibrates(m) ? range_guard_recalibrate : range_guard_rerun)(m, s, x_dev, x_dtype, batch, y_dev, 0, nullptr, nullptr, nullptr));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return 0;
}

int c3_model_range_status(c3_model *m, int *flag_out, int *on_fp32_out) {
    if (!m) return fail("null model");
    HIP_TRY(hipSetDevice(m->device));
    uint32_t f = 0;
    HIP_TRY(hipDeviceSynchronize());
    TRY(d2h_staged(&f, m->range_flag, 4));
    if (flag_out) *flag_out = (int)f;
    if (on_fp32_out) *on_fp32_out = m->f16_ok ? 0 : 1;
    return 0;
}

int c3_model_set_sharing(c3_model *m, int handles) {
    if (!m) return fail("null model");
    if (handles < 1) return fail("handles must be >= 1");
    m->sharing = handles;
    return 0;
}

int c3_model_describe(c3_model *m, char *buf, int n) {
    if (!m || !buf || n <= 0) return fail("null argument");
    // plane_stores: the build's C3_PLANE_STORE_AUX (c3_gemm.h), so that the log of a same-box comparison names the build.  Second field, not
    // last: the suite looks at the last field of both strings (chunks / pack_rows, ",layers:1")
    static const char *const stores = C3_PLANE_STORE_AUX == 16 ? "write-through" : "default";
    if (m->kind == C3_KIND_PILEUP)
        snprintf(buf, (size_t)n, "sharing=%d plane_stores=%s lstm1=%s proj2=%s lstm2=%s on_fp32=%d precision=%s lstm_wmax=%.4g lstm_hh_norm=%.4g auto_fp32_at=%.4g "
                 "ring_lanes=%d lane_max_batch=%lld max_depth=%d rescaled=%lld candidates=%lld kept=%lld chunks=%lld", m->sharing,
                 stores, m->choice.lstm1, m->choice.proj2, m->choice.lstm2, (int)!m->f16_ok, m->answer_exact ? "exact" : m->precision, (double)m->lstm_wmax, (double)m->lstm_hh_norm,
                 (double)(m->precision_forced ? 0.f : m->auto_fp32_at), m->ring_lanes, (long long)m->lane_max_batch, m->max_depth,
                 (long long)m->rescaled, (long long)m->cand_n, (long long)m->cand_kept, (long long)m->cand_chunks);
    else {
        // wino_form: the form of every F(2,3) layer of the last pass (c3_conv3w.h), res2a:paired/res2b:paired/res3a:transform-waves, "-" without
        // one; fa_tail: the FC chain of the last pass (c3_forward.h run_tail).  The row counters stay the last three fields, pack_rows the last one
        static const char *const names[6] = {"res1a", "res1b", "res2a", "res2b", "res3a", "res3b"};
        char wf[160] = "";
        for (int i = 0; i < 6; ++i)
            if (m->choice.s1[i] == 'w') {
                const size_t at = strlen(wf);
                snprintf(wf + at, sizeof(wf) - at, "%s%s:%s", at ? "/" : "", names[i], m->choice.wform[i] == 't' ? "transform-waves" : "paired");
            }
        // wave_prio: the convolutions of the last pass that ran a wave priority scheme (c3_forward.h run_fa_planes), conv3/res2a/res2b, "-" for none
        char wp[96] = "";
        for (int l = 1; l < 9; ++l)
            if (m->choice.prio >> l & 1u) {
                const size_t at = strlen(wp);
                snprintf(wp + at, sizeof(wp) - at, "%s%s", at ? "/" : "", kFaLayerTag[l] + 3);  // ("fa.res2a" -> "res2a")
            }
        snprintf(buf, (size_t)n, "sharing=%d plane_stores=%s conv_stack=%s stride1=%s conv3=%s conv5=%s on_fp32=%d ring_lanes=%d lane_max_batch=%lld "
                 "precision=%s wino_form=%s fa_tail=%s wave_prio=%s rows_windows=%lld rows_shipped=%lld pack_rows=%d", m->sharing,
                 stores, m->choice.fa, m->choice.s1, m->choice.s2[0], m->choice.s2[1], (int)!m->f16_ok, m->ring_lanes, (long long)m->lane_max_batch,
                 m->answer_exact ? "exact" : m->precision, wf[0] ? wf : "-", m->choice.fa_tail, wp[0] ? wp : "-", (long long)m->rows_windows, (long long)m->rows_shipped, (int)m->pack_rows);
    }
    if (m->fp32_plan | m->fp32_auto) {  // only while a precision plan is in force (c3_model.h layer_f16)
        const size_t at = strlen(buf);
        snprintf(buf + at, (size_t)n - at, " fp32_layers=%s", layer_mask_text(m->kind, m->fp32_plan | m->fp32_auto).c_str());
    }
    if (m->lowering_set) {  // only while a lowering is set (c3_calibrate.h)
        const size_t at = strlen(buf);
        snprintf(buf + at, (size_t)n - at, " calibration=cap:%d,windows:%lld,lowered:%d", m->lowering_cap, (long long)m->lowering_windows,
                 (int)std::count_if(m->lowering, m->lowering + kCalChannels, [](uint8_t v) { return v != 0; }));
    }
    if (m->range_policy != C3_RANGE_STICKY) {  // only while a range-guard policy other than sticky is set (c3_calibrate.h)
        const size_t at = strlen(buf);
        snprintf(buf + at, (size_t)n - at, " range_guard=recalibrate,recalibrations:%lld%s", (long long)m->rstats.recalibrations, m->rstats.fell_back ? ",fell_back" : "");
    }
    if (m->verify_seen) {  // verify mode is or was on (c3_verify.h): the setting and the totals behind everything else
        const c3_verify_stats &t = m->vstats;
        const size_t at = strlen(buf);
        snprintf(buf + at, (size_t)n - at, " verify=every:%d,policy:%s,tol:%.3g,submitted:%lld,checked:%lld,skipped:%lld,windows:%lld,max_abs_diff:%.3g,"
                 "rows_over_tol:%lld,label_diffs:%lld,near_ties:%lld,escalations:%lld", m->verify_every,
                 m->verify_policy == C3_VERIFY_ESCALATE ? "escalate" : m->verify_policy == C3_VERIFY_REPLACE ? "replace" : "report", (double)m->verify_tol, (long long)t.batches_submitted,
                 (long long)t.batches_checked, (long long)t.batches_skipped, (long long)t.windows_checked, (double)t.max_abs_diff,
                 (long long)t.rows_over_tol, (long long)(t.label_diffs[0] + t.label_diffs[1] + t.label_diffs[2] + t.label_diffs[3]),
                 (long long)(t.near_ties[0] + t.near_ties[1] + t.near_ties[2] + t.near_ties[3]), (long long)t.escalations);
        if (m->verify_layers) snprintf(buf + strlen(buf), (size_t)n - strlen(buf), ",layers:1");
        if (m->verify_ref == C3_VERIFY_REF_EXACT) snprintf(buf + strlen(buf), (size_t)n - strlen(buf), ",ref:exact");  // only while the reference is the exact form
    }
    if (m->exact.want) snprintf(buf + strlen(buf), (size_t)n - strlen(buf), " exact=1");  // only while the exact form is enabled (c3_exact.h)
    if (m->score_on)  // only while score mode is enabled (c3_score.h)
        snprintf(buf + strlen(buf), (size_t)n - strlen(buf), " score=gamma:%g,weights:%d%s", m->score_gamma, (int)m->score_weighted,
                 m->score_census_on ? ",census:1" : "");
    if (m->refine_on)  // only while refine mode is on (c3_refine.h)
        snprintf(buf + strlen(buf), (size_t)n - strlen(buf), " refine=gap:%g,windows:%lld,selected:%lld,changed:%lld", (double)m->refine_gap,
                 (long long)m->rfstats.windows, (long long)m->rfstats.windows_selected, (long long)m->rfstats.windows_changed);
    return 0;
}

int c3_model_synchronize(c3_model *m) {
    if (!m) return fail("null model");
    for (const Lane &L : m->lanes)
        if (L.stream) HIP_TRY(hipStreamSynchronize(L.stream));
    return 0;
}

int c3_model_destroy(c3_model *m) {
    if (!m) return 0;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    free_all_workspaces(m);
    exact_free_workspace(m);
    exact_free_weights(m);
    if (m->exact.ring_ev) (void)hipEventDestroy(m->exact.ring_ev);
    for (const Lane &L : m->lanes)
        if (L.stream) (void)hipStreamDestroy(L.stream);
    float *ws[] = {m->proj_w[0], m->proj_w[1], m->proj_b[0], m->proj_b[1], m->whh[0], m->whh[1], m->whh16[0], m->whh16[1],
                   m->l4_w, m->l4_b, m->l4_wf, m->b5, m->zeros, m->l1_wih, m->l1_wih16, m->l1_bias, m->conv1_w16,
                   m->conv1_wfrag16, m->w5f, m->whf, m->bh48, m->proj2_pw, m->proj2_pwr, m->proj2_post, m->conv1_post,
                   m->conv1_w16_post, m->l4_pre, m->l4_post};
    for (float *p : ws)
        if (p) (void)hipFree(p);
    if (m->decode_dev) (void)hipFree(m->decode_dev);
    for (float *p : m->tap_dev)
        if (p) (void)hipFree(p);
    if (m->range_flag) (void)hipFree(m->range_flag);
    if (m->layer_exp) (void)hipFree(m->layer_exp);
    if (m->census_dev) (void)hipFree(m->census_dev);
    if (m->refine_rows) (void)hipFree(m->refine_rows);
    if (m->variant_dev) (void)hipFree(m->variant_dev);
    if (m->pin_flag) (void)hipHostFree(m->pin_flag);
    for (int l = 0; l < 9; ++l) {
        if (m->conv_w[l]) (void)hipFree(m->conv_w[l]);
        if (m->conv_b[l]) (void)hipFree(m->conv_b[l]);
        if (m->pconv_w[l]) (void)hipFree(m->pconv_w[l]);
        if (m->pconv_pre[l]) (void)hipFree(m->pconv_pre[l]);
        if (m->pconv_post[l]) (void)hipFree(m->pconv_post[l]);
        if (m->wconv_w[l]) (void)hipFree(m->wconv_w[l]);
        if (m->wconv_post[l]) (void)hipFree(m->wconv_post[l]);
    }
    for (auto &sl : m->slot) {
        if (sl.pin_x) (void)hipHostFree(sl.pin_x);
        if (sl.pin_y) (void)hipHostFree(sl.pin_y);
        if (sl.pin_flag) (void)hipHostFree(sl.pin_flag);
        if (sl.dev_x) (void)hipFree(sl.dev_x);
        if (sl.dev_y) (void)hipFree(sl.dev_y);
        if (sl.shadow) (void)hipFree(sl.shadow);
        if (sl.layer_part) (void)hipFree(sl.layer_part);
        if (sl.score_part) (void)hipFree(sl.score_part);
        if (sl.refine_scratch) (void)hipFree(sl.refine_scratch);
        for (float *p : sl.layer_buf)
            if (p) (void)hipFree(p);
        if (sl.ev_h2d) (void)hipEventDestroy(sl.ev_h2d);
        if (sl.ev_out) (void)hipEventDestroy(sl.ev_out);
    }
    for (auto &r : m->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    if (m->h2d_stream) (void)hipStreamDestroy(m->h2d_stream);
    delete m;
    return 0;
}

}  // extern "C"
