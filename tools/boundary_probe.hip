// tools/boundary_probe.hip -- what does a dependent kernel boundary cost behind B bytes of freshly stored output, and do write-through
// (sc1) stores take that cost away?  (run on the GPU box; C3_PLANE_STORE_AUX in clair3_amd/csrc/c3_gemm.h is the decision it prices)
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 tools/boundary_probe.hip -o /tmp/bp && /tmp/bp
// Two kernels on one stream:
//   A<AUX>  512 workgroups x 256 threads (two per CU, as the plane convolutions).  Each wave stores whole 128-byte lines with 16-byte buffer
//           stores -- 8 lanes x 16 B = one line, 1 KB contiguous per instruction: the pattern of the plane epilogues -- B bytes in all,
//           with aux 0 (default policy) or 16 (sc1), spread evenly over a fixed stream of matrix instructions that makes the launch
//           last about 40 us, as the layers do;
//   B       a trivial dependent kernel, one wave per CU, that reads one word per MB of what A stored.
// After a 60 ms ramp, device events around 200 back-to-back (A, B) pairs, five times: us per pair (min / median / max) for
// B in {0, 4, 8, 16, 27, 50} MB x {plain, sc1}, and the same for A alone (a slower store path would show there).  If the release at the
// end of A writes back what A left dirty in the eight 4 MB L2s, the plain pair grows with B up to the L2s' capacity and the sc1 pair
// stays flat.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int kWgs = 512, kThreads = 256;
constexpr int kMfmas = 1200;  // per wave, two waves per SIMD: 2 x 1200 x 32 cycles = 77 k cycles, about 40 us at the sustained clock

template <int AUX>
__global__ __launch_bounds__(kThreads, 2) void store_kernel(char *out, uint32_t bytes, uint32_t *flag) {
    // num_records = bytes: a piece beyond the end vanishes in the bounds check of the buffer store
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(out, 0, bytes, 0x00020000);
    const uint32_t sweep = (uint32_t)(kWgs * kThreads) * 16u;  // bytes all threads store with one instruction each
    int sweeps = (int)((bytes + sweep - 1) / sweep);
    const int interval = kMfmas / (sweeps > 0 ? sweeps : 1);
    uint32_t off = (uint32_t)(blockIdx.x * kThreads + threadIdx.x) * 16u;
    f16x8 a = __builtin_bit_cast(f16x8, u32x4{threadIdx.x, blockIdx.x, 0x3c003c00u, 0x3c003c00u});
    f32x16 c = {};
    int until = interval;
    for (int k = 0; k < kMfmas; ++k) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, a, c, 0, 0, 0);
        if (--until == 0) {
            until = interval;
            if (sweeps > 0) {
                --sweeps;
                const u32x4 v = {(uint32_t)k, off, __float_as_uint(c[0]), __float_as_uint(c[5])};
                __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, off, 0, AUX);
                off += sweep;
            }
        }
    }
    if (c[3] == 77.f) flag[0] = 1;
}

__global__ __launch_bounds__(64) void read_kernel(const uint32_t *in, int mb, uint32_t *flag) {
    const int t = threadIdx.x;
    const uint32_t v = t < mb ? in[(size_t)t << 18] : 0u;
    if (v == 0xdeadbeefu && blockIdx.x == 1u << 20) flag[1] = 1;
}

struct Stat { float lo, med, hi; };

template <int AUX>
static int measure(char *buf, int mb, uint32_t *flag, bool pair, Stat *st) {
    const uint32_t bytes = (uint32_t)mb << 20;
    auto launch = [&]() {
        hipLaunchKernelGGL(store_kernel<AUX>, dim3(kWgs), dim3(kThreads), 0, 0, buf, bytes, flag);
        if (pair) hipLaunchKernelGGL(read_kernel, dim3(256), dim3(64), 0, 0, (const uint32_t *)buf, mb, flag);
    };
    const auto t0 = std::chrono::steady_clock::now();
    do {  // ramp: 60 ms of the same work
        for (int i = 0; i < 100; ++i) launch();
        CK(hipDeviceSynchronize());
    } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 0.060);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float us[5];
    for (int r = 0; r < 5; ++r) {
        CK(hipEventRecord(e0));
        for (int i = 0; i < 200; ++i) launch();
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        us[r] = ms * 1e3f / 200.f;
    }
    CK(hipGetLastError());
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    std::sort(us, us + 5);
    *st = {us[0], us[2], us[4]};
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    printf("%s, %d CUs; A = %d workgroups x %d threads, %d matrix instructions per wave; 200 launches (pairs) per figure, 5 figures: min / median / max in us\n",
           prop.gcnArchName, prop.multiProcessorCount, kWgs, kThreads, kMfmas);
    const int sizes[] = {0, 4, 8, 16, 27, 50};
    char *buf;
    uint32_t *flag;
    CK(hipMalloc(&buf, (size_t)64 << 20));
    CK(hipMalloc(&flag, 256));
    CK(hipMemset(buf, 0, (size_t)64 << 20));
    CK(hipMemset(flag, 0, 256));
    printf("%6s | %-26s | %-26s | %-26s | %-26s | %s\n", "MB", "pair (A, B) plain", "pair (A, B) sc1", "A alone plain", "A alone sc1", "median pair plain - sc1");
    for (int mb : sizes) {
        Stat pp, ps, ap, as;
        if (measure<0>(buf, mb, flag, true, &pp) || measure<16>(buf, mb, flag, true, &ps)) return 1;
        if (measure<0>(buf, mb, flag, false, &ap) || measure<16>(buf, mb, flag, false, &as)) return 1;
        printf("%6d | %7.2f %7.2f %7.2f    | %7.2f %7.2f %7.2f    | %7.2f %7.2f %7.2f    | %7.2f %7.2f %7.2f    | %+6.2f\n", mb, pp.lo, pp.med, pp.hi, ps.lo,
               ps.med, ps.hi, ap.lo, ap.med, ap.hi, as.lo, as.med, as.hi, pp.med - ps.med);
        fflush(stdout);
    }
    CK(hipFree(buf));
    CK(hipFree(flag));
    return 0;
}
