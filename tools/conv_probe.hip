// tools/conv_probe.hip -- phase ablation of conv3x3_planes_kernel (run on the GPU box):
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -I clair3_amd/csrc tools/conv_probe.hip -o /tmp/conv_probe && /tmp/conv_probe
// Times the kernel on the three residual-block shapes of a B = 256 full-alignment batch, whole and with parts switched off (ABL
// bits: 1 no weight loads, 2 no halo loads after the first tile, 4 no epilogue, 8 no matrix instructions), at one and two
// workgroups per CU, with the second workgroup of a CU started later (skew), and prints a shader-clock trace of workgroups 0 and
// 256 (the two that share a CU: tools/census_probe.hip).  Numbers only -- correctness is the parity tests' job.
//   conv_probe prio   the wave priority schemes (c3_conv3.h wave_prio_step) on res1 (1530 tiles on 512 workgroups) and on res3b with the
//                     pooling epilogue (512 tiles): start / end stamps of every workgroup and the launch time per scheme, alternating
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../clair3_amd/csrc/c3_conv3.h"
#include "stamp_report.h"
using namespace c3;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

template <class K>
static float time_it(K launch, int reps = 20) {
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    launch(); launch(); hipDeviceSynchronize();
    hipEventRecord(a); for (int i = 0; i < reps; ++i) launch(); hipEventRecord(b); hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b); return ms / reps * 1e3f;
}
template <int C, int ABL> static float run(const PlaneConvParams &cp, int grid) {
    return time_it([&] { hipLaunchKernelGGL((conv3x3_planes_kernel<C, true, ABL>), dim3(grid), dim3(kPlThreads), 0, 0, cp); });
}
template <int C, bool SPPF, int ABL> static void launch_p(const PlaneConvParams &cp, int grid) {
    hipLaunchKernelGGL((conv3x3_planes_kernel<C, true, ABL, 0, SPPF>), dim3(grid), dim3(kPlThreads), 0, 0, cp);
}
template <int C, bool SPPF = false> static int shape(const char *name, int B, int H, int W, int cus, bool prio = false) {
    constexpr int NS = C / 64;
    const size_t bytes = (size_t)B * H * W * C * 4;
    void *x, *y, *r, *wf; float *bias, *post; uint32_t *flag;
    CK(hipMalloc(&x, bytes)); CK(hipMalloc(&y, bytes)); CK(hipMalloc(&r, bytes));
    CK(hipMalloc(&wf, (size_t)9 * C * C * 4)); CK(hipMalloc(&bias, C * 4)); CK(hipMalloc(&post, C * 4)); CK(hipMalloc(&flag, 256));
    // realistic plane activations: post-ReLU values (a third of them zero) as genuine hi / lo fp16 pairs -- the power draw of
    // a matrix instruction (and with it the clock the chip sustains) depends on how many operand bits toggle
    std::vector<_Float16> h(bytes / 2);
    for (size_t g = 0; g < h.size() / 128; ++g)  // one (pixel, slab) group: [hi 64][lo 64]
        for (int c = 0; c < 64; ++c) {
            const uint32_t u = (uint32_t)((g * 64 + c) * 2654435761u);
            const float xv = (u % 3 == 0) ? 0.f : (float)(u >> 8) / 16777216.f * 3.f;
            const _Float16 hi = (_Float16)xv;
            h[g * 128 + c] = hi, h[g * 128 + 64 + c] = (_Float16)(xv - (float)hi);
        }
    CK(hipMemcpy(x, h.data(), bytes, hipMemcpyHostToDevice)); CK(hipMemcpy(r, h.data(), bytes, hipMemcpyHostToDevice));
    std::vector<uint16_t> hw((size_t)9 * C * C * 2);  // any fragment order will do for timing: genuine hi / lo pairs per 16-byte piece pair
    for (size_t g = 0; g < hw.size() / 1024; ++g)   // [hi: 64 lanes x 8][lo: 64 lanes x 8]
        for (int c = 0; c < 512; ++c) {
            const uint32_t u = (uint32_t)((g * 512 + c) * 40503u + 12345u) * 2654435761u;
            const float xv = ((float)(u >> 8) / 16777216.f - 0.5f) * 8.f;  // folded weights times the packing scale
            const _Float16 hi = (_Float16)xv, lo = (_Float16)(xv - (float)hi);
            memcpy(&hw[g * 1024 + c], &hi, 2), memcpy(&hw[g * 1024 + 512 + c], &lo, 2);
        }
    CK(hipMemcpy(wf, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    std::vector<float> hb(C, 0.f), hp(C, 1.f / 4096.f);
    CK(hipMemcpy(bias, hb.data(), C * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(post, hp.data(), C * 4, hipMemcpyHostToDevice)); CK(hipMemset(flag, 0, 256));
    PlaneConvParams cp;
    cp.x = x, cp.wf = wf, cp.bias = bias, cp.res = r, cp.out = y, cp.range_flag = flag, cp.post = post, cp.pre = post;
    cp.M = B * H * W, cp.H = H, cp.W = W;
    cp.mg_hw = (uint32_t)((1ull << 32) / (uint64_t)(H * W) + 1), cp.mg_w = (uint32_t)((1ull << 32) / (uint64_t)W + 1);  // fast_div magics
    const int tiles_m = (cp.M + kPlBM - 1) / kPlBM;
    cp.tiles = tiles_m * NS;
    const int unit = 8 * NS;
    auto grid_for = [&](int s) { return cp.tiles <= s ? cp.tiles : s / unit * unit; };
    const int g = grid_for(2 * cus);
    if (prio) {
        float *spp = nullptr;
        if constexpr (SPPF) {  // (c3_forward.h run_fa_planes: two whole windows per tile, the pooled bins instead of planes)
            CK(hipMalloc((void **)&spp, (size_t)B * 14 * C * 4));
            cp.spp = spp, cp.tiles = (B + 1) / 2 * NS;
        }
        const int gp = grid_for(2 * cus);
        long long *tb; CK(hipMalloc(&tb, (size_t)2 * gp * 8));
        cp.trace = tb, cp.cus = cus;
        printf("== %s%s: M = %d, %d tiles on %d workgroups, %d CUs; schemes: 0 none, 1 younger workgroup at priority 1 for the first half of its slabs, "
               "2 both alternate per slab, 3 both alternate per weight chunk\n", name, SPPF ? " with the pooling epilogue" : "", cp.M, cp.tiles, gp, cus);
        const int steps = (cp.tiles + gp - 1) / gp * NS;  // slabs of the tiles of a workgroup's walk
        auto set_scheme = [&](int scheme) {  // 3: per chunk (ABL bit 256: bit 0 of the mask is the phase)
            if (scheme < 3) wave_prio_masks(scheme, steps, cp.prio);
            else cp.prio[0] = kPrioOn, cp.prio[1] = kPrioOn | 1u;
        };
        for (int scheme = 0; scheme < 4; ++scheme) {
            set_scheme(scheme);
            CK(hipMemset(tb, 0, (size_t)2 * gp * 8));
            std::vector<long long> ht((size_t)2 * gp);
            printf("  scheme %d, first start to last end of six launches (us):", scheme);
            for (int k = 0; k < 6; ++k) {  // (the last launch is the one reported in full)
                if (scheme < 3) launch_p<C, SPPF, 128>(cp, gp);
                else launch_p<C, SPPF, 128 | 256>(cp, gp);
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(ht.data(), tb, ht.size() * 8, hipMemcpyDeviceToHost));
                printf(" %.2f", stamp_span(ht, gp));
            }
            printf("\n");
            char what[32]; snprintf(what, sizeof what, "scheme %d, one launch:", scheme);
            stamp_report(what, ht, gp, cus);
        }
        for (int rep = 0; rep < 5; ++rep) {
            printf("  launch time, 200 launches back to back (us), schemes 0 1 2 3:");
            for (int scheme = 0; scheme < 4; ++scheme) {
                set_scheme(scheme);
                printf(" %6.2f", scheme < 3 ? time_it([&] { launch_p<C, SPPF, 0>(cp, gp); }, 200) : time_it([&] { launch_p<C, SPPF, 256>(cp, gp); }, 200));
            }
            printf("\n");
        }
        hipFree(tb); hipFree(spp);
        hipFree(x); hipFree(y); hipFree(r); hipFree(wf); hipFree(bias); hipFree(post); hipFree(flag);
        return 0;
    }
    const double mf = 2.0 * tiles_m * kPlBM * (double)C * 9.0 * C * 3;
    printf("== %s: M = %d, %d tiles of %d pixels, grid %d; executed matrix work %.1f GFLOP = %.1f us at 2500 TF; in+out+res %.0f MB\n", name, cp.M, cp.tiles, kPlBM, g,
           mf / 1e9, mf / 2500e6, 3 * bytes / 1e6);
    printf("  full                         %6.1f us\n", run<C, 0>(cp, g));
    printf("  no weight loads              %6.1f us\n", run<C, 1>(cp, g));
    printf("  no halo loads                %6.1f us\n", run<C, 2>(cp, g));
    printf("  no epilogue                  %6.1f us\n", run<C, 4>(cp, g));
    printf("  no loads, no epilogue        %6.1f us\n", run<C, 7>(cp, g));
    printf("  no MFMA                      %6.1f us\n", run<C, 8>(cp, g));
    printf("  full, one workgroup per CU   %6.1f us (grid %d)\n", run<C, 0>(cp, grid_for(cus)), grid_for(cus));
    for (int skew : {4, 8, 16}) {
        cp.skew = skew;
        printf("  full, skew %2d x 1024 cycles  %6.1f us\n", skew, run<C, 0>(cp, g));
    }
    cp.skew = 0;
    {   // shader-clock trace of workgroups 0 and 256, wave 0 (RES = false: p.res is the trace buffer)
        long long *tb; CK(hipMalloc(&tb, 2 * 256 * 16)); CK(hipMemset(tb, 0, 2 * 256 * 16));
        PlaneConvParams ct = cp;
        ct.res = tb;
        hipLaunchKernelGGL((conv3x3_planes_kernel<C, false, 64>), dim3(g), dim3(kPlThreads), 0, 0, ct);
        hipLaunchKernelGGL((conv3x3_planes_kernel<C, false, 64>), dim3(g), dim3(kPlThreads), 0, 0, ct);
        CK(hipDeviceSynchronize());
        std::vector<long long> ht(2 * 256 * 2);
        CK(hipMemcpy(ht.data(), tb, ht.size() * 8, hipMemcpyDeviceToHost));
        for (int wg = 0; wg < 2; ++wg) {
            printf("  trace workgroup %d (tag:+cycles; 2 first loads issued 3 prologue done 10+tap chunk done 30 tile done 31 staged 32 stored 33 next halo in):\n   ", wg ? 256 : 0);
            for (int i = 1; i < 250 && ht[(wg * 256 + i) * 2] != 0; ++i)
                printf(" %lld:+%lld", ht[(wg * 256 + i) * 2], ht[(wg * 256 + i) * 2 + 1] - ht[(wg * 256 + i - 1) * 2 + 1]);
            printf("\n");
        }
        hipFree(tb);
    }
    hipFree(x); hipFree(y); hipFree(r); hipFree(wf); hipFree(bias); hipFree(post); hipFree(flag);
    return 0;
}
int main(int argc, char **argv) {
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    if (argc > 1 && !strcmp(argv[1], "prio")) {
        if (shape<64>("res1", 256, 45, 17, cus, true)) return 1;
        if (shape<256, true>("res3b", 256, 12, 5, cus, true)) return 1;
        return 0;
    }
    if (shape<64>("res1", 256, 45, 17, cus)) return 1;
    if (shape<128>("res2", 256, 23, 9, cus)) return 1;
    if (shape<256>("res3", 256, 12, 5, cus)) return 1;
    return 0;
}
