// launch_dwt3.hip -- launchers of the depth-axis DWT level kernels of a volume (dwt3_axis_kernels.hpp).
//
// Columns per thread: 16 B per lane (four fp32, two fp64 columns) for filters of at most 16 taps, half of that for 18-40 taps
// (the register window is HLEN x columns values), whenever the slice length is a multiple of it and both buffers are aligned
// to it; else one column per lane.  One instantiation per even filter length and width, like the other families.
#include "launch.hpp"
#include "launch_util.hpp"

#include "dwt3_axis_kernels.hpp"

namespace pdwt {

int dwt3_depth_width(const void* in, const void* out, long long P, int hlen) { return dwt3_width(in, out, P, hlen); }

int dwt3_depth_steps(int Nz, int hlen, bool inverse) { return inverse ? dwt3_inv_steps(Nz, hlen) : dwt3_fwd_steps(Nz); }

int dwt3_depth_seg(int Nz, long long P, int hlen, int width, bool inverse, int slots) {
    return dwt3_pick_seg(dwt3_depth_steps(Nz, hlen, inverse), dwt3_col_groups(P, width), hlen, slots);
}

template <int HLEN, bool INV>
static hipError_t run_depth(const Dwt3Args& a, int width, hipStream_t s) {
    constexpr int W = dwt3_wide(HLEN);
    const long long gx = dwt3_col_groups(a.P, width);
    const int gy = cdiv(dwt3_depth_steps(a.Nz, HLEN, INV), a.seg);
    if (gx > 0x7fffffffLL || gy > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)gy), block(kDwt3NT);
    if constexpr (W > 1) {
        if (width == W) {
            if constexpr (INV) hipLaunchKernelGGL((dwt3_depth_inv_kernel<HLEN, W>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((dwt3_depth_fwd_kernel<HLEN, W>), grid, block, 0, s, a);
            return hipGetLastError();
        }
    }
    if (width != 1) return hipErrorInvalidValue;
    if constexpr (INV) hipLaunchKernelGGL((dwt3_depth_inv_kernel<HLEN, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((dwt3_depth_fwd_kernel<HLEN, 1>), grid, block, 0, s, a);
    return hipGetLastError();
}

// workgroups of one instantiation the chip keeps resident (the runtime's occupancy answer x CUs, asked once per kernel)
template <int HLEN, bool INV>
static int resident_depth(int width) {
    constexpr int W = dwt3_wide(HLEN);
    static std::atomic<int> wide{0}, narrow{0};
    if constexpr (W > 1) {
        if (width == W) {
            if constexpr (INV) return resident_slots(dwt3_depth_inv_kernel<HLEN, W>, kDwt3NT, 0, &wide);
            else return resident_slots(dwt3_depth_fwd_kernel<HLEN, W>, kDwt3NT, 0, &wide);
        }
    }
    if constexpr (INV) return resident_slots(dwt3_depth_inv_kernel<HLEN, 1>, kDwt3NT, 0, &narrow);
    else return resident_slots(dwt3_depth_fwd_kernel<HLEN, 1>, kDwt3NT, 0, &narrow);
}

int dwt3_depth_slots(int hlen, int width, bool inverse) {
    switch (hlen) {
#define X(h) case h: return inverse ? resident_depth<h, true>(width) : resident_depth<h, false>(width);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return 0;
}

template <bool INV>
static hipError_t launch_depth(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg,
                               hipStream_t s) {
    if (!in || !out || Nz < 1 || P < 1 || seg < 1) return hipErrorInvalidValue;
    Dwt3Args a;
    a.in = in;
    a.out = out;
    a.Nz = Nz;
    a.Nh = dwt3_div2(Nz);
    a.P = P;
    a.seg = seg;
    a.fb = fb;
    const int width = dwt3_depth_width(in, out, P, hlen);
    switch (hlen) {
#define X(h) case h: return run_depth<h, INV>(a, width, s);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return hipErrorNotSupported;
}

hipError_t launch_dwt3_depth_fwd(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_depth<false>(in, out, Nz, P, hlen, fb, seg, s);
}

hipError_t launch_dwt3_depth_inv(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_depth<true>(in, out, Nz, P, hlen, fb, seg, s);
}

}  // namespace pdwt
