// c3_debug.h -- introspection for the parity tests and bench.py: per-layer activations of the last forward pass, HIP-event
// timing of every launch on the launch stream.  Not needed by a pipeline.
#pragma once
#include "c3_forward.h"

// n floats of debug tensor `s` at src (device) as the checkpoint's fp32 values on the host: plane activations (c3_conv3.h) converted,
// the channel powers of two of the full-alignment activations (channel equalisation, c3_pack.h) removed.  The caller has synchronised the device.
static int to_host_values(c3_model *m, const std::string &s, const float *src, int64_t n, bool planes, float *host_out) {
    const std::vector<int> *exps = nullptr;
    if (m->kind == C3_KIND_FULL_ALIGNMENT && s.compare(0, 3, "act") == 0) exps = &m->act_exp[s[3] - '0'];
    if (m->kind == C3_KIND_FULL_ALIGNMENT && s == "spp") exps = &m->act_exp[8];
    auto unscale = [&]() {
        if (!exps || exps->empty()) return;
        const size_t C = exps->size();
        for (int64_t i = 0; i < n; ++i) host_out[i] = std::ldexp(host_out[i], -(*exps)[(size_t)i % C]);
    };
    if (planes) {
        const int C = m->kind == C3_KIND_PILEUP ? 256 : kConvCout[s[3] - '0'];
        float *tmp = nullptr;
        HIP_TRY(hipMalloc((void **)&tmp, (size_t)n * sizeof(float)));
        hipLaunchKernelGGL(planes_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const void *)src, tmp, n / C, C);
        const int rc = d2h_staged(host_out, tmp, (size_t)n * sizeof(float));
        (void)hipFree(tmp);
        if (rc != 0) return rc;
        unscale();
        return 0;
    }
    TRY(d2h_staged(host_out, src, (size_t)n * sizeof(float)));
    unscale();
    return 0;
}

extern "C" {

int c3_debug_keep_activations(c3_model *m, int enable) {
    if (!m) return fail("null model");
    HIP_TRY(hipSetDevice(m->device));
    if (m->keep != (enable != 0)) {
        HIP_TRY(hipStreamSynchronize(lane(m).stream));
        free_workspace(lane(m));
        m->keep = enable != 0;
    }
    return 0;
}

int c3_debug_fetch(c3_model *m, const char *name, float *host_out, int64_t n_floats) {
    if (!m || !name || !host_out) return fail("null argument");
    HIP_TRY(hipSetDevice(m->device));
    const Lane &L = lane(m);
    if (L.last_n <= 0) return fail("nothing has been predicted yet");
    const std::string s = name;
    const float *src = nullptr;
    int64_t n = 0;
    if (m->kind == C3_KIND_PILEUP) {
        if (s == "lstm1_out") src = L.h1, n = L.last_n * m->positions * 256;
        else if (s == "lstm2_out") src = L.h2, n = L.last_n * m->positions * 320;
        else if (s == "gx2") src = L.gx2, n = L.last_n * m->positions * 1280;
    } else {
        int hh[10], ww[10];
        fa_geometry(m, hh, ww);
        if (s.size() == 4 && s.compare(0, 3, "act") == 0 && s[3] >= '0' && s[3] <= '8') {
            if (!m->keep) return fail("activations are recycled: enable c3_debug_keep_activations first");
            const int l = s[3] - '0';
            src = L.act[l], n = L.last_n * hh[l + 1] * ww[l + 1] * kConvCout[l];
        } else if (s == "spp") src = L.spp, n = L.last_n * m->K4;
    }
    if (s == "l4_out") {
        if (!m->keep) return fail("l4_out is only written with c3_debug_keep_activations enabled");
        src = L.l4dbg, n = L.last_n * m->FC;
    }
    if (!src) return fail("unknown debug tensor \"%s\"", name);
    if (n != n_floats) return fail("debug tensor %s has %lld floats, caller expects %lld", name, (long long)n, (long long)n_floats);
    HIP_TRY(hipDeviceSynchronize());
    const bool planes = L.last_planes && ((m->kind == C3_KIND_FULL_ALIGNMENT && s.compare(0, 3, "act") == 0) || (m->kind == C3_KIND_PILEUP && s == "lstm1_out"));
    return to_host_values(m, s, src, n, planes, host_out);
}

// c3_debug_tap: tensors by name, comma separated ("" = none)
int c3_debug_tap(c3_model *m, const char *names) {
    if (!m || !names) return fail("null argument");
    HIP_TRY(hipSetDevice(m->device));
    uint32_t mask = 0;
    std::string list = names;
    for (size_t a = 0; a < list.size();) {
        size_t b = list.find(',', a);
        if (b == std::string::npos) b = list.size();
        const std::string name = list.substr(a, b - a);
        a = b + 1;
        if (name.empty()) continue;
        int id = -1;
        for (int i = 0; i < kTapCount; ++i)
            if (name == kTapName[i]) id = i;
        const bool fa_tensor = id >= 0 && id <= kTapL4, p_tensor = id >= kTapL4;
        if (id < 0 || (m->kind == C3_KIND_FULL_ALIGNMENT ? !fa_tensor : !p_tensor))
            return fail("unknown tap tensor \"%s\" for the %s network", name.c_str(), m->kind == C3_KIND_PILEUP ? "pileup" : "full-alignment");
        mask |= 1u << id;
    }
    HIP_TRY(hipDeviceSynchronize());
    for (int id = 0; id < kTapCount; ++id) {
        if ((mask >> id & 1u) || !m->tap_dev[id]) continue;
        (void)hipFree(m->tap_dev[id]);
        m->tap_dev[id] = nullptr, m->tap_bytes[id] = 0;
    }
    m->tap_mask = mask;
    m->tap_written = m->tap_skipped = m->tap_planes = 0, m->tap_n = 0;
    return 0;
}

int c3_debug_tap_fetch(c3_model *m, const char *name, int64_t first, int64_t windows, float *host_out, int64_t n_floats) {
    if (!m || !name || (!host_out && n_floats > 0)) return fail("null argument");
    HIP_TRY(hipSetDevice(m->device));
    int id = -1;
    for (int i = 0; i < kTapCount; ++i)
        if (!strcmp(name, kTapName[i])) id = i;
    if (id < 0 || !(m->tap_mask >> id & 1u)) return fail("%s is not tapped: c3_debug_tap first", name);
    if (m->tap_skipped >> id & 1u) {
        if (id == 0) return fail("act0 is computed inside res1a (conv1 inside the first residual block): the form writes no act0");
        if (id == 8) return fail("act8 is pooled inside res3b (the pyramid pooling is its epilogue): the form writes no act8");
        return fail("%s was not produced by the last call's form", name);
    }
    if (!(m->tap_written >> id & 1u) || m->tap_n <= 0) return fail("%s: no call since it was tapped", name);
    if (first < 0 || windows < 0 || first + windows > m->tap_n)
        return fail("windows %lld .. %lld of %s: the last call had %lld", (long long)first, (long long)(first + windows), name, (long long)m->tap_n);
    const int64_t pw = tap_window_floats(m, id), n = windows * pw;
    if (n != n_floats) return fail("%lld windows of %s are %lld floats, caller expects %lld", (long long)windows, name, (long long)n, (long long)n_floats);
    if (n == 0) return 0;
    HIP_TRY(hipDeviceSynchronize());
    return to_host_values(m, name, m->tap_dev[id] + first * pw, n, (m->tap_planes >> id & 1u) != 0, host_out);
}

int c3_profile_enable(c3_model *m, int enable) {
    if (!m) return fail("null model");
    m->prof = enable != 0;
    return 0;
}

int c3_profile_reset(c3_model *m) {
    if (!m) return fail("null model");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    for (auto &r : m->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    m->recs.clear();
    return 0;
}

int c3_profile_read(c3_model *m, c3_kernel_stat *out, int max_entries) {
    if (!m || (!out && max_entries > 0)) {
        fail("null argument");
        return -1;
    }
    if (hipSetDevice(m->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        fail("device synchronize failed");
        return -1;
    }
    std::vector<std::string> order;
    std::map<std::string, c3_kernel_stat> agg;
    for (auto &r : m->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
        auto it = agg.find(r.name);
        if (it == agg.end()) {
            c3_kernel_stat st;
            memset(&st, 0, sizeof(st));
            snprintf(st.name, sizeof(st.name), "%s", r.name.c_str());
            it = agg.insert({r.name, st}).first;
            order.push_back(r.name);
        }
        it->second.launches += 1;
        it->second.total_ms += ms;
        it->second.flops += r.flops;
        it->second.bytes += r.bytes;
        it->second.mfma_flops += r.mfma_flops;
        it->second.mfma_peak_tflops = std::max(it->second.mfma_peak_tflops, r.mfma_peak);
    }
    int n = 0;
    for (auto &k : order) {
        if (n >= max_entries) break;
        out[n++] = agg[k];
    }
    return (int)order.size();
}

}  // extern "C"
