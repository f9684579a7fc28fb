// axis_common.hpp -- what the two depth-axis kernel families of a volume (dwt3_axis_kernels.hpp, swt3_axis_kernels.hpp), their
// launchers (launch_depth3.hip) and their emulations (tests/cpu_emu/emu_axis.cpp, emu_swt_axis.cpp) share: the access shape.  A
// thread owns VEC neighbouring columns of a plane of P samples and walks along the depth; gridDim.x = column groups.
#pragma once

#include "kernels_common.hpp"

namespace pdwt {

// index math, host and device; with -DPDWT_CPU_EMU the tile functions run on the host
#ifdef PDWT_CPU_EMU
#define PDWT_HD static inline
#else
#define PDWT_HD static __host__ __device__ __forceinline__
#endif

constexpr int kAxisNT = 256;        // threads per workgroup
constexpr int kAxisTapsInLds = 18;  // from this filter length on the taps are staged in LDS, not held in scalar registers

// the columns per thread a launch takes: `wide` where the slice length is a multiple of it and both buffers are aligned to it, else 1
static inline int axis_width(const void* in, const void* out, long long P, int wide) {
    const uintptr_t mask = (uintptr_t)wide * sizeof(real_t) - 1;
    const bool ok = wide > 1 && P % wide == 0 && !(reinterpret_cast<uintptr_t>(in) & mask) && !(reinterpret_cast<uintptr_t>(out) & mask);
    return ok ? wide : 1;
}
static inline long long axis_col_groups(long long P, int width) { return (P + (long long)kAxisNT * width - 1) / ((long long)kAxisNT * width); }

// ---- VEC columns of one slice -----------------------------------------------------------------------------------------

template <int VEC>
struct alignas(VEC * sizeof(real_t)) AxisVec {
    real_t v[VEC];
};

template <int VEC>
PDWT_DEVICE AxisVec<VEC> axis_load(const real_t* PDWT_RESTRICT base, long long slice, long long P, long long col) {
    return *reinterpret_cast<const AxisVec<VEC>*>(base + slice * P + col);
}

template <int VEC>
PDWT_DEVICE void axis_store(real_t* PDWT_RESTRICT base, long long slice, long long P, long long col, const AxisVec<VEC>& x) {
    *reinterpret_cast<AxisVec<VEC>*>(base + slice * P + col) = x;
}

}  // namespace pdwt
