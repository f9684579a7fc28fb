// launch_depth3.hip -- launchers of the depth-axis level kernels of a volume: the decimated ones (dwt3_axis_kernels.hpp) and the
// a-trous ones of a stationary volume (swt3_axis_kernels.hpp), through one template over a traits struct per transform.
//
// Columns per thread: the transform's wide(hlen, inverse) -- 16 B per lane while the register window leaves room, then 8 B, then
// one column (dwt3_wide, swt3_wide) -- whenever the slice length is a multiple of it and both buffers are aligned to it; else one
// column per lane.  One instantiation per even filter length, direction and width, like the other families.
#include "launch.hpp"
#include "launch_util.hpp"

#include "dwt3_axis_kernels.hpp"
#include "swt3_axis_kernels.hpp"

namespace pdwt {

namespace {

// per transform: the argument struct, the kernel of an <HLEN, W, INV>, the wide width and gridDim.y of a launch
struct Dwt3 {
    using Args = Dwt3Args;
    static constexpr int wide(int hlen, bool) { return dwt3_wide(hlen); }
    static long long grid_y(const Args& a, int hlen, bool inverse) { return cdiv(dwt3_depth_steps(a.Nz, hlen, inverse), a.seg); }
    template <int HLEN, int W, bool INV>
    static constexpr auto kernel() {
        if constexpr (INV) return &dwt3_depth_inv_kernel<HLEN, W>;
        else return &dwt3_depth_fwd_kernel<HLEN, W>;
    }
};

struct Swt3 {
    using Args = Swt3Args;
    static constexpr int wide(int hlen, bool inverse) { return swt3_wide(hlen, inverse); }
    static long long grid_y(const Args& a, int, bool) { return (long long)a.orbits * a.nseg; }
    template <int HLEN, int W, bool INV>
    static constexpr auto kernel() {
        if constexpr (INV) return &swt3_depth_inv_kernel<HLEN, W>;
        else return &swt3_depth_fwd_kernel<HLEN, W>;
    }
};

template <class T, int HLEN, bool INV>
hipError_t run_depth(const typename T::Args& a, int width, hipStream_t s) {
    constexpr int W = T::wide(HLEN, INV);
    const long long gx = axis_col_groups(a.P, width), gy = T::grid_y(a, HLEN, INV);
    if (gx > 0x7fffffffLL || gy > 65535 || (width != W && width != 1)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)gy), block(kAxisNT);
    if (width == W) hipLaunchKernelGGL((T::template kernel<HLEN, W, INV>()), grid, block, 0, s, a);
    else hipLaunchKernelGGL((T::template kernel<HLEN, 1, INV>()), grid, block, 0, s, a);
    return hipGetLastError();
}

// workgroups of one instantiation the chip keeps resident (the runtime's occupancy answer x CUs, asked once per kernel)
template <class T, int HLEN, bool INV>
int resident_depth(int width) {
    constexpr int W = T::wide(HLEN, INV);
    static std::atomic<int> wide{0}, narrow{0};
    if (W > 1 && width == W) return resident_slots(T::template kernel<HLEN, W, INV>(), kAxisNT, 0, &wide);
    return resident_slots(T::template kernel<HLEN, 1, INV>(), kAxisNT, 0, &narrow);
}

template <class T>
int depth_slots(int hlen, int width, bool inverse) {
    switch (hlen) {
#define X(h) case h: return inverse ? resident_depth<T, h, true>(width) : resident_depth<T, h, false>(width);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return 0;
}

template <class T, bool INV>
hipError_t launch_depth(const typename T::Args& a, int hlen, hipStream_t s) {
    const int width = axis_width(a.in, a.out, a.P, T::wide(hlen, INV));
    switch (hlen) {
#define X(h) case h: return run_depth<T, h, INV>(a, width, s);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return hipErrorNotSupported;
}

template <bool INV>
hipError_t launch_dwt3(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg, hipStream_t s) {
    if (!in || !out || Nz < 1 || P < 1 || seg < 1) return hipErrorInvalidValue;
    Dwt3Args a;
    a.in = in;
    a.out = out;
    a.Nz = Nz;
    a.Nh = dwt3_div2(Nz);
    a.P = P;
    a.seg = seg;
    a.fb = fb;
    return launch_depth<Dwt3, INV>(a, hlen, s);
}

template <bool INV>
hipError_t launch_swt3(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg, hipStream_t s) {
    if (!in || !out || Nz < 1 || P < 1 || f < 1 || seg < 1) return hipErrorInvalidValue;
    Swt3Args a;
    a.in = in;
    a.out = out;
    a.P = P;
    a.fb = fb;
    swt3_geometry(a, Nz, f, seg);
    return launch_depth<Swt3, INV>(a, hlen, s);
}

}  // namespace

// ---- the decimated transform
int dwt3_depth_width(const void* in, const void* out, long long P, int hlen) { return dwt3_width(in, out, P, hlen); }

int dwt3_depth_steps(int Nz, int hlen, bool inverse) { return inverse ? dwt3_inv_steps(Nz, hlen) : dwt3_fwd_steps(Nz); }

int dwt3_depth_seg(int Nz, long long P, int hlen, int width, bool inverse, int slots) {
    return dwt3_pick_seg(dwt3_depth_steps(Nz, hlen, inverse), dwt3_col_groups(P, width), hlen, slots);
}

int dwt3_depth_slots(int hlen, int width, bool inverse) { return depth_slots<Dwt3>(hlen, width, inverse); }

hipError_t launch_dwt3_depth_fwd(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_dwt3<false>(in, out, Nz, P, hlen, fb, seg, s);
}

hipError_t launch_dwt3_depth_inv(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_dwt3<true>(in, out, Nz, P, hlen, fb, seg, s);
}

// ---- the stationary transform
int swt3_depth_width(const void* in, const void* out, long long P, int hlen, bool inverse) { return swt3_width(in, out, P, hlen, inverse); }

int swt3_depth_steps(int Nz, int f) { return Nz >= 1 && f >= 1 ? swt3_steps(f, Nz) : 0; }

int swt3_depth_seg(int Nz, int f, long long P, int hlen, int width, int slots) {
    if (Nz < 1 || f < 1) return 1;
    return swt3_pick_seg(swt3_steps(f, Nz), swt3_col_groups(P, width), swt3_orbits(f, Nz), hlen, slots);
}

int swt3_depth_slots(int hlen, int width, bool inverse) { return depth_slots<Swt3>(hlen, width, inverse); }

hipError_t launch_swt3_depth_fwd(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_swt3<false>(in, out, Nz, P, f, hlen, fb, seg, s);
}

hipError_t launch_swt3_depth_inv(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s) {
    return launch_swt3<true>(in, out, Nz, P, f, hlen, fb, seg, s);
}

}  // namespace pdwt
