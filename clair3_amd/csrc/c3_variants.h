// c3_variants.h -- what the three variant instruments share (jackknife, subsample and occlusion mode: c3_jackknife.h, c3_subsample.h,
// c3_occlude.h; DESIGN.md 4, "The variant pass"): a window's input is staged once, its variants are built on the device from a table, base
// windows and variants go through the unchanged forward pass, their rows are reduced to records, and the records come home in one copy per
// pass.  Host code only, no kernel: the pass and its cut, the layout of a pass in the handle's one variant buffer, the forms of the handle for
// one call, the driver with its range-guard retry, and what the entries refuse alike.  A mode supplies its entry struct, its kernels, its
// plan, and a small struct of five operations (variant_run below says which).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

namespace c3 {

// A call is cut into passes of `chunk` windows (0: one pass); a window's variants never straddle a pass.
struct VariantPass {
    int64_t w0 = 0, windows = 0;     // the windows [w0, w0 + windows) of the call
    int64_t unit0 = 0, units = 0;    // their staged units in the caller's input: occupied rows (full alignment), windows (pileup)
    int64_t var0 = 0, variants = 0;  // their variants among the call's: [var0, var0 + variants)
    int64_t dense() const { return windows + variants; }  // dense windows the pass builds: base windows first, then every variant
};
// env `name`: windows per pass, 0 = never cut; unset or negative: dflt
static inline int64_t variant_chunk_env(const char *name, int64_t dflt) {
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : dflt;
    return v < 0 ? dflt : (int64_t)v;
}
// count: the windows' occupied rows, or null: one unit a window (pileup).  variants_of(w): the variants of window w of the call
template <class VariantsOf>
static inline std::vector<VariantPass> variant_cut(const int32_t *count, int64_t batch, int64_t chunk, VariantsOf variants_of) {
    std::vector<VariantPass> out;
    int64_t unit = 0, var = 0;
    for (int64_t w = 0; w < batch;) {
        VariantPass ps;
        ps.w0 = w, ps.windows = chunk > 0 ? std::min(chunk, batch - w) : batch - w, ps.unit0 = unit, ps.var0 = var;
        for (int64_t i = 0; i < ps.windows; ++i) ps.units += count ? count[w + i] : 1, ps.variants += variants_of(w + i);
        out.push_back(ps);
        w += ps.windows, unit += ps.units, var += ps.variants;
    }
    return out;
}
// where a pass's sections sit in the handle's variant buffer, every section from a multiple of 256 bytes: the staged input | the meta block
// (the mode's table and what else its kernels read) | the rows y of the dense windows | "home": the records that come home in one copy, with
// the pass's 4-byte copy of the range flag directly behind them | an optional extra section (drops, masks).  What lies inside the meta block
// and inside home is the mode's own
struct VariantLayout {
    size_t unit_bytes = 0, meta_bytes = 0, home_bytes = 0;
    size_t in_at = 0, meta_at = 0, meta_end = 0;                         // staged
    size_t y_at = 0, home_at = 0, flag_at = 0, extra_at = 0, bytes = 0;  // written by the device
    VariantLayout(const VariantPass &ps, size_t unit_bytes_, size_t meta_bytes_, int row_floats, size_t home_bytes_, size_t extra_bytes)
        : unit_bytes(unit_bytes_), meta_bytes(meta_bytes_), home_bytes(home_bytes_) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        meta_at = al((size_t)ps.units * unit_bytes);
        meta_end = meta_at + meta_bytes;
        y_at = al(meta_end);
        home_at = al(y_at + (size_t)ps.dense() * row_floats * sizeof(float));
        flag_at = home_at + home_bytes;  // (every record is a multiple of 4 bytes)
        extra_at = al(flag_at + 4);
        bytes = extra_at + extra_bytes;
    }
};
// the meta block of the two modes whose windows have runs of reads (jackknife, subsample), offsets within the block: the table of
// entry_bytes a dense window | every window's first variant (int64) | its count (int32), each from a multiple of 256 bytes
struct RunMeta {
    size_t var_first_at = 0, count_at = 0, bytes = 0;
    RunMeta(const VariantPass &ps, size_t entry_bytes) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        var_first_at = al((size_t)ps.dense() * entry_bytes);
        count_at = al(var_first_at + (size_t)ps.windows * sizeof(int64_t));
        bytes = count_at + (size_t)ps.windows * sizeof(int32_t);
    }
};

}  // namespace c3

// what a call did, as the driver fills it: c3_jackknife_info, c3_subsample_info and c3_occlude_info (include/c3hip.h) field for field
struct VariantInfo {
    int64_t windows, variants, passes, bytes_staged;
    int32_t on_fp32, reserved;
    float expand_us, reduce_us;
};
#define C3_VARIANT_INFO_IS(T)                                                                                                                    \
    static_assert(sizeof(T) == sizeof(VariantInfo) && offsetof(T, windows) == offsetof(VariantInfo, windows) &&                                   \
                      offsetof(T, variants) == offsetof(VariantInfo, variants) && offsetof(T, passes) == offsetof(VariantInfo, passes) &&         \
                      offsetof(T, bytes_staged) == offsetof(VariantInfo, bytes_staged) && offsetof(T, on_fp32) == offsetof(VariantInfo, on_fp32) && \
                      offsetof(T, expand_us) == offsetof(VariantInfo, expand_us) && offsetof(T, reduce_us) == offsetof(VariantInfo, reduce_us),   \
                  #T " has the layout of VariantInfo")
C3_VARIANT_INFO_IS(c3_jackknife_info);
C3_VARIANT_INFO_IS(c3_subsample_info);
C3_VARIANT_INFO_IS(c3_occlude_info);

// the handle's variant buffer: one pass of one call at a time (every entry is blocking and refuses a handle with a prediction in flight);
// grown, never shrunk
static int ensure_variant_buf(c3_model *m, size_t bytes) {
    if (m->variant_bytes >= bytes) return 0;
    HIP_TRY(hipDeviceSynchronize());
    if (m->variant_dev) (void)hipFree(m->variant_dev);
    m->variant_dev = nullptr, m->variant_bytes = 0;
    HIP_TRY(hipMalloc(&m->variant_dev, bytes));
    m->variant_bytes = bytes;
    return 0;
}
// the active lane's buffer of dense pileup windows that occlusion mode builds (occlude_pileup_expand_kernel), sized like the lane's buffer of
// rescaled windows (ensure_rescale_buf): as many int32 windows as its workspace holds; allocated on first use, grown, freed with the workspace
static int ensure_occlude_window_buf(c3_model *m) {
    Lane &L = lane(m);
    if (L.xo && L.xo_cap >= L.cap) return 0;
    HIP_TRY(hipDeviceSynchronize());
    if (L.xo) (void)hipFree(L.xo);
    L.xo = nullptr, L.xo_cap = 0;
    HIP_TRY(hipMalloc(&L.xo, std::max<size_t>((size_t)L.cap * m->positions * m->C * sizeof(int32_t), 256)));
    L.xo_cap = L.cap;
    return 0;
}

// HIP events around the launches of one kind, only for a caller that asks for the info struct: mark() in front of and behind each launch
struct VariantTimer {
    bool on = false;
    std::vector<hipEvent_t> ev;
    void mark(hipStream_t s) {
        hipEvent_t e;
        if (!on || hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, s);
        ev.push_back(e);
    }
    float total_us() {  // behind the stream's last synchronisation; destroys the events
        float us = 0.f;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) us += ms * 1e3f;
        }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
        return us;
    }
};
// one launch of `blocks` workgroups between two marks of the timer (null: no marks); nothing for blocks <= 0
template <class Kernel, class Params>
static int variant_launch(hipStream_t s, VariantTimer *timer, Kernel kernel, int64_t blocks, int threads, const Params &p) {
    if (blocks <= 0) return 0;
    if (timer) timer->mark(s);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)threads), 0, s, p);
    HIP_TRY(hipGetLastError());
    if (timer) timer->mark(s);
    return 0;
}

// The forms the handle is on, for one call alone: between enter() and leave() forward passes are enqueued on the handle's forms (attempt 0)
// or on the fp32 forms (attempt 1) without taps or profile records; leave() puts back what the handle reports, taps, profiles and counts.
// A field of the handle that a pass must leave alone is added HERE.  (c3_calibrate.h keeps its own: it always runs the fp32 forms, sets
// census_pass and leaves tap_mask standing.)
struct FormsForCall {
    c3_model *m;
    const c3_model::Choices choice;
    const bool f16_ok, tap_call, prof;
    const int64_t tap_base;
    const uint32_t tap_mask;
    explicit FormsForCall(c3_model *m_)
        : m(m_), choice(m_->choice), f16_ok(m_->f16_ok), tap_call(m_->tap_call), prof(m_->prof), tap_base(m_->tap_base), tap_mask(m_->tap_mask) {}
    void enter(int attempt) { m->f16_ok = attempt == 0 ? f16_ok : false, m->tap_call = true, m->prof = false, m->tap_mask = 0; }
    void leave() { m->f16_ok = f16_ok, m->tap_call = tap_call, m->prof = prof, m->tap_base = tap_base, m->tap_mask = tap_mask, m->choice = choice; }
};

// the dense windows of a pass, micro-batch by micro-batch through the forms the handle is on, their rows at y (row stride m->row).  The mode
// builds a micro-batch into the lane's buffer of expanded full-alignment windows, or of dense pileup windows; int8 and int32 pileup windows
// stay on their own kernels, as in forward_device
template <class Mode>
static int variant_forward(c3_model *m, hipStream_t s, const Mode &mode, const int8_t *in, const char *meta, char *extra, int64_t total, int x_dtype,
                           float *y, VariantTimer &timer) {
    TRY(ensure_workspace(m, total));
    const bool fa = m->kind == C3_KIND_FULL_ALIGNMENT;
    if (fa) TRY(ensure_expand_buf(m));
    else TRY(ensure_occlude_window_buf(m));
    Lane &L = lane(m);
    for (int64_t off = 0; off < total; off += L.cap) {
        const int64_t n = std::min<int64_t>(L.cap, total - off);
        TRY(mode.expand(s, timer, in, meta, extra, off, n, fa ? (void *)L.xe : L.xo));
        float *yp = y + off * m->row;
        if (fa) TRY(run_fa(m, s, L.xe, n, yp));
        else if (x_dtype == C3_DTYPE_I8) TRY(run_pileup_t<int8_t>(m, s, (const int8_t *)L.xo, n, yp));
        else TRY(run_pileup_t<int32_t>(m, s, (const int32_t *)L.xo, n, yp));
        L.last_n = n;
    }
    return 0;
}

// The driver of a call.  in_host: the staged units of the call back to back (full alignment: the occupied rows; pileup: the windows
// themselves); passes: its cut.  A mode is a struct with
//   chunk_var                                         the name of its environment switch, for the message below
//   layout(ps)                                        the VariantLayout of a pass
//   fill(meta, ps)                                    the meta block of a pass as it is staged, every byte of layout(ps).meta_bytes
//   expand(s, timer, in, meta, extra, off, n, dst)    the launch that builds dense windows [off, off + n) of the pass at dst
//   reduce(s, timer, ps, L, base)                     the launch that reduces the pass's rows to its records
//   deliver(s, ps, home, extra)                       a pass's records (host bytes) and its extra section (device) into the caller's arrays
// Per pass: stage, then at most two attempts.  On a full-alignment handle that is on the fp16x3 forms the first attempt is guarded: a scan
// of the rows raises bit 1 of the range flag for a non-finite row as in the ring, and the pass's copy of the flag comes home behind the
// records -- the one place the host waits for the pass.  A flag that is up puts the device flag back to zero and runs THIS PASS again on the
// fp32-MFMA forms, which do not look at it.  A pileup handle has no such guard.
template <class Mode>
static int variant_run(c3_model *m, const char *who, const int8_t *in_host, int x_dtype, const std::vector<VariantPass> &passes, const Mode &mode,
                       float *y_host, float *variant_rows_out, void *info) {
    size_t need = 0;
    for (const VariantPass &ps : passes) {
        if (ps.dense() > INT32_MAX) return fail("%s: %lld dense windows in one pass: set %s", who, (long long)ps.dense(), Mode::chunk_var);
        need = std::max(need, mode.layout(ps).bytes);
    }
    HIP_TRY(hipSetDevice(m->device));
    TRY(use_lane(m, 0));
    hipStream_t s = lane(m).stream;
    TRY(ensure_variant_buf(m, need));
    const bool fa = m->kind == C3_KIND_FULL_ALIGNMENT;
    FormsForCall forms(m);
    VariantInfo did = {};
    int rc = 0;
    VariantTimer t_expand, t_reduce;
    t_expand.on = t_reduce.on = info != nullptr;
    std::vector<char> meta, home;
    char *base = (char *)m->variant_dev;
    for (const VariantPass &ps : passes) {
        const VariantLayout L = mode.layout(ps);
        meta.resize(L.meta_bytes);
        mode.fill(meta.data(), ps);
        if (ps.units) rc = h2d_staged(base + L.in_at, in_host + (size_t)ps.unit0 * L.unit_bytes, (size_t)ps.units * L.unit_bytes, s);
        if (rc == 0) rc = h2d_staged(base + L.meta_at, meta.data(), meta.size(), s);
        if (rc) break;
        did.bytes_staged += (int64_t)((size_t)ps.units * L.unit_bytes + meta.size());
        float *y = (float *)(base + L.y_at);
        for (int attempt = 0; attempt < 2 && rc == 0; ++attempt) {
            const bool guarded = fa && forms.f16_ok && attempt == 0;
            forms.enter(attempt);
            rc = variant_forward(m, s, mode, (const int8_t *)(base + L.in_at), base + L.meta_at, base + L.extra_at, ps.dense(), x_dtype, y, t_expand);
            forms.leave();
            if (rc) break;
            if (guarded) {
                const int64_t nf = ps.dense() * m->row;
                hipLaunchKernelGGL(rows_finite_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, y, nf, m->range_flag);
                if (hipGetLastError() != hipSuccess) {
                    rc = fail("%s: the scan of the rows could not be launched", who);
                    break;
                }
            }
            if ((rc = mode.reduce(s, t_reduce, ps, L, base)) != 0) break;
            if (guarded && hipMemcpyAsync(base + L.flag_at, m->range_flag, 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
                rc = fail("%s: hipMemcpyAsync failed", who);
                break;
            }
            home.resize(L.home_bytes + (guarded ? 4 : 0));
            if ((rc = d2h_staged(home.data(), base + L.home_at, home.size(), s)) != 0) break;
            uint32_t flag = 0;
            if (guarded) memcpy(&flag, home.data() + L.home_bytes, 4);
            if (flag) {  // beyond the range of the fp16x3 kernels: this pass again on the fp32-MFMA forms, for this call alone
                if (hipMemsetAsync(m->range_flag, 0, 256, s) != hipSuccess) rc = fail("%s: hipMemsetAsync failed", who);
                did.on_fp32 = 1;
                continue;
            }
            if (y_host) rc = d2h_staged(y_host + ps.w0 * m->row, y, (size_t)ps.windows * m->row * sizeof(float), s);
            if (rc == 0) rc = mode.deliver(s, ps, home.data(), base + L.extra_at);
            if (rc == 0 && variant_rows_out && ps.variants)
                rc = d2h_staged(variant_rows_out + ps.var0 * m->row, y + ps.windows * m->row, (size_t)ps.variants * m->row * sizeof(float), s);
            break;
        }
        if (rc) break;
        did.windows += ps.windows, did.variants += ps.variants, ++did.passes;
    }
    if (rc) {
        const std::string why = g_err;
        (void)hipStreamSynchronize(s);
        (void)t_expand.total_us(), (void)t_reduce.total_us();
        return g_err = why, rc;
    }
    did.expand_us = t_expand.total_us(), did.reduce_us = t_reduce.total_us();  // (the last copy home has synchronised the stream)
    if (info) memcpy(info, &did, sizeof(did));
    return 0;
}

// ------------------------------------------------------------------------------------------ what the entries share
// what every entry that runs the network refuses before anything is queued.  fa_only: null, or the refusal of a pileup handle (one %s: who)
static int variant_handle(c3_model *m, const char *who, const char *fa_only) {
    if (!m) return fail("null model");
    if (fa_only && m->kind != C3_KIND_FULL_ALIGNMENT) return fail(fa_only, who);
    for (const HostSlot &sl : m->slot)
        if (sl.busy) return fail("%s: a prediction is in flight: call c3_predict_wait first", who);
    if (m->answer_exact) return fail("%s: the handle answers from the exact form: c3_model_set_answer(m, C3_ANSWER_PRODUCT) first", who);
    if (!m->loaded) return fail("model has no weights: call c3_model_load first");
    return 0;
}
// row_first (null: the centring rule) / row_count of a rows entry -> one checked first / count per window, and the rows in all
static int checked_runs(c3_model *m, const int32_t *row_first, const int32_t *row_count, int64_t batch, std::vector<int32_t> *first,
                        std::vector<int32_t> *count, int64_t *total) {
    first->resize((size_t)batch), count->resize((size_t)batch);
    *total = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const int32_t c = table_i32(row_count, b);
        if (c < 0) return fail("window %lld: negative row_count %d", (long long)b, c);
        const int32_t f = row_first ? table_i32(row_first, b) : (m->depth - c) / 2;
        if (f < 0) return fail("window %lld: negative row_first %d", (long long)b, f);
        if ((int64_t)f + c > m->depth)
            return fail("window %lld: rows [%d, %lld) reach beyond the depth of %d rows", (long long)b, f, (long long)f + c, m->depth);
        (*first)[(size_t)b] = f, (*count)[(size_t)b] = c, *total += c;
    }
    return 0;
}
// dense full-alignment windows of a dense entry -> every window's run, found on the host as c3_pack_rows finds it (its first row is the
// run's own), and the runs' rows back to back: only the occupied rows are staged
static void gather_runs(c3_model *m, const void *x_host, int64_t batch, std::vector<int32_t> *first, std::vector<int32_t> *count, std::vector<int8_t> *rows) {
    const size_t row_bytes = (size_t)m->positions * m->C, wbytes = (size_t)m->depth * row_bytes;
    first->resize((size_t)batch), count->resize((size_t)batch);
    size_t total = 0;
    for (int64_t b = 0; b < batch; ++b) {
        occupied_run((const uint8_t *)x_host + (size_t)b * wbytes, m->depth, row_bytes, &(*first)[(size_t)b], &(*count)[(size_t)b]);
        total += (size_t)(*count)[(size_t)b];
    }
    rows->resize(std::max<size_t>(total * row_bytes, 1));
    size_t at = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const size_t n = (size_t)(*count)[(size_t)b] * row_bytes;
        memcpy(rows->data() + at, (const char *)x_host + (size_t)b * wbytes + (size_t)(*first)[(size_t)b] * row_bytes, n);
        at += n;
    }
}
