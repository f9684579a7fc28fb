// volshiftbench.hip -- times the circular-shift kernels of a volume on their own (developer tool, not part of the library).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I pypwt_amd/csrc tools/volshiftbench.hip -o tools/bin/volshiftbench
//   tools/bin/volshiftbench Nz Nr Nc [reps] [warmup]          (tools/volbench.py --spin builds and runs it)
// vol_circshift_kernel and vol_unshift_acc_kernel (pypwt_amd/csrc/volume_shift_kernels.hpp, launched as launch_volume_ops.hip
// launches them) by HIP events after a warm-up, every line twice, with a column shift of 4 (groups both ways where Nc % 4 == 0)
// and of 3 (groups stored, values loaded).  Next to each, in the same run, the flat 16-B grid-stride copy of the same bytes -- the
// library's copy_kernel, 1024 workgroups: one volume copied moves the shift's two volumes, one and a half the accumulate's three.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <functional>

#include "volume_shift_kernels.hpp"

using namespace pdwt;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

__global__ void __launch_bounds__(256) copy4(const float4* __restrict__ a, float4* __restrict__ b, long long n4) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) b[i] = a[i];
}

__global__ void fill(float* x, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = (float)((i * 2654435761u) >> 8 & 0xffff) * (1.0f / 256.0f);
}

static float time_ms(hipEvent_t a, hipEvent_t b, const std::function<void()>& fn, int reps, int warmup) {
    for (int i = 0; i < warmup; i++) fn();
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < reps; i++) fn();
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    CK(hipGetLastError());
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

static void shift(const float* in, float* out, const VolShiftGeom& g) {
    const dim3 grid(vol_shift_grid(g)), block(kVolShiftThreads);
    if (g.mode == 2) hipLaunchKernelGGL(vol_circshift_kernel<2>, grid, block, 0, 0, in, out, g);
    else if (g.mode == 1) hipLaunchKernelGGL(vol_circshift_kernel<1>, grid, block, 0, 0, in, out, g);
    else hipLaunchKernelGGL(vol_circshift_kernel<0>, grid, block, 0, 0, in, out, g);
}

static void unshift_acc(const float* rec, float* acc, const VolShiftGeom& g) {
    const dim3 grid(vol_shift_grid(g)), block(kVolShiftThreads);
    if (g.mode == 2) hipLaunchKernelGGL(vol_unshift_acc_kernel<2>, grid, block, 0, 0, rec, acc, g, 0.125f, 0);
    else if (g.mode == 1) hipLaunchKernelGGL(vol_unshift_acc_kernel<1>, grid, block, 0, 0, rec, acc, g, 0.125f, 0);
    else hipLaunchKernelGGL(vol_unshift_acc_kernel<0>, grid, block, 0, 0, rec, acc, g, 0.125f, 0);
}

int main(int argc, char** argv) {
    if (argc < 4) return printf("usage: volshiftbench Nz Nr Nc [reps] [warmup]\n"), 2;
    const int Nz = atoi(argv[1]), Nr = atoi(argv[2]), Nc = atoi(argv[3]);
    const int reps = argc > 4 ? atoi(argv[4]) : 50, warmup = argc > 5 ? atoi(argv[5]) : 5;
    if (Nz < 1 || Nr < 1 || Nc < 1 || reps < 1) return 2;
    const long long n = (long long)Nz * Nr * Nc, half = (n * 3 / 2) & ~3LL;
    float *a = nullptr, *b = nullptr;
    CK(hipMalloc((void**)&a, (size_t)(half + 4) * sizeof(float)));
    CK(hipMalloc((void**)&b, (size_t)(half + 4) * sizeof(float)));
    hipLaunchKernelGGL(fill, dim3(1024), dim3(256), 0, 0, a, half);
    hipLaunchKernelGGL(fill, dim3(1024), dim3(256), 0, 0, b, half);
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const double vol = (double)n * sizeof(float);
    auto copy = [&](long long elems) {
        const long long n4 = elems / 4;
        long long grid = (n4 + 255) / 256;
        if (grid > 1024) grid = 1024;
        hipLaunchKernelGGL(copy4, dim3((unsigned)grid), dim3(256), 0, 0, reinterpret_cast<const float4*>(a), reinterpret_cast<float4*>(b), n4);
    };
    auto line = [&](const char* what, int mode, const std::function<void()>& fn, double bytes, float yard) {
        const float t0 = time_ms(e0, e1, fn, reps, warmup), t1 = time_ms(e0, e1, fn, reps, warmup);
        const float t = t0 < t1 ? t0 : t1;
        char share[32] = "";
        if (yard > 0) snprintf(share, sizeof(share), "  %.2f of the copy", yard / t);
        printf("  %dx%dx%d  %-40s mode %d %10.4f %10.4f ms %8.0f GB/s%s\n", Nz, Nr, Nc, what, mode, t0, t1, bytes / (t * 1e6), share);
        return t;
    };
    const float c2 = line("flat copy, 1 volume (2 moved)", -1, [&] { copy(n & ~3LL); }, 2 * vol, 0);
    const float c3 = line("flat copy, 1.5 volumes (3 moved)", -1, [&] { copy(half); }, 3 * vol, 0);
    for (int sc : {4, 3}) {
        char what[64];
        const VolShiftGeom g = vol_shift_geom_of(Nz, Nr, Nc, 1, 2, sc, false, a, b);
        snprintf(what, sizeof(what), "vol_circshift (1, 2, %d)", sc);
        line(what, g.mode, [&] { shift(a, b, g); }, 2 * vol, c2);
        const VolShiftGeom u = vol_shift_geom_of(Nz, Nr, Nc, 1, 2, sc, true, a, b);
        snprintf(what, sizeof(what), "vol_unshift_acc (1, 2, %d)", sc);
        line(what, u.mode, [&] { unshift_acc(a, b, u); }, 3 * vol, c3);
    }
    CK(hipFree(a));
    CK(hipFree(b));
    return 0;
}
