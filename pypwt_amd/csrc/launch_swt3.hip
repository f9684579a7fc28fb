// launch_swt3.hip -- launchers of the depth-axis a-trous kernels of a stationary volume (swt3_axis_kernels.hpp).
//
// Columns per thread: swt3_wide(hlen, inverse) -- 16 B per lane while the register window (HLEN slices forward, 2 HLEN inverse)
// leaves room, then 8 B, then one column -- whenever the slice length is a multiple of it and both buffers are aligned to it; else
// one column per lane.  One instantiation per even filter length, direction and width, like the other families.
#include "launch.hpp"
#include "launch_util.hpp"

#include "swt3_axis_kernels.hpp"

namespace pdwt {

int swt3_depth_width(const void* in, const void* out, long long P, int hlen, bool inverse) { return swt3_width(in, out, P, hlen, inverse); }

int swt3_depth_steps(int Nz, int f) { return Nz >= 1 && f >= 1 ? swt3_steps(f, Nz) : 0; }

int swt3_depth_seg(int Nz, int f, long long P, int hlen, int width, int slots) {
    if (Nz < 1 || f < 1) return 1;
    return swt3_pick_seg(swt3_steps(f, Nz), swt3_col_groups(P, width), swt3_orbits(f, Nz), hlen, slots);
}

template <int HLEN, bool INV>
static hipError_t run_depth(const Swt3Args& a, int width, hipStream_t s) {
    constexpr int W = swt3_wide(HLEN, INV);
    const long long gx = swt3_col_groups(a.P, width);
    const long long gy = (long long)a.orbits * a.nseg;
    if (gx > 0x7fffffffLL || gy > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)gy), block(kSwt3NT);
    if constexpr (W > 1) {
        if (width == W) {
            if constexpr (INV) hipLaunchKernelGGL((swt3_depth_inv_kernel<HLEN, W>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((swt3_depth_fwd_kernel<HLEN, W>), grid, block, 0, s, a);
            return hipGetLastError();
        }
    }
    if (width != 1) return hipErrorInvalidValue;
    if constexpr (INV) hipLaunchKernelGGL((swt3_depth_inv_kernel<HLEN, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((swt3_depth_fwd_kernel<HLEN, 1>), grid, block, 0, s, a);
    return hipGetLastError();
}

// workgroups of one instantiation the chip keeps resident (the runtime's occupancy answer x CUs, asked once per kernel)
template <int HLEN, bool INV>
static int resident_depth(int width) {
    constexpr int W = swt3_wide(HLEN, INV);
    static std::atomic<int> wide{0}, narrow{0};
    if constexpr (W > 1) {
        if (width == W) {
            if constexpr (INV) return resident_slots(swt3_depth_inv_kernel<HLEN, W>, kSwt3NT, 0, &wide);
            else return resident_slots(swt3_depth_fwd_kernel<HLEN, W>, kSwt3NT, 0, &wide);
        }
    }
    if constexpr (INV) return resident_slots(swt3_depth_inv_kernel<HLEN, 1>, kSwt3NT, 0, &narrow);
    else return resident_slots(swt3_depth_fwd_kernel<HLEN, 1>, kSwt3NT, 0, &narrow);
}

int swt3_depth_slots(int hlen, int width, bool inverse) {
    switch (hlen) {
#define X(h) case h: return inverse ? resident_depth<h, true>(width) : resident_depth<h, false>(width);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return 0;
}

template <bool INV>
static hipError_t launch_depth(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg,
                               hipStream_t s) {
    if (!in || !out || Nz < 1 || P < 1 || f < 1 || seg < 1) return hipErrorInvalidValue;
    Swt3Args a;
    a.in = in;
    a.out = out;
    a.P = P;
    a.fb = fb;
    swt3_geometry(a, Nz, f, seg);
    const int width = swt3_depth_width(in, out, P, hlen, INV);
    switch (hlen) {
#define X(h) case h: return run_depth<h, INV>(a, width, s);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return hipErrorNotSupported;
}

hipError_t launch_swt3_depth_fwd(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_depth<false>(in, out, Nz, P, f, hlen, fb, seg, s);
}

hipError_t launch_swt3_depth_inv(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_depth<true>(in, out, Nz, P, f, hlen, fb, seg, s);
}

}  // namespace pdwt
