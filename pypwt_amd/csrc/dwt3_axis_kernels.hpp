// dwt3_axis_kernels.hpp -- one decimated DWT level along the SLOWEST axis of a volume (the depth pass of pdwt_volume,
// volume.cpp).  The reference has no 3D transform ("3D is not handled at the moment", pdwt/README.md:29; its constructor stops
// at ndim == 3, pdwt/src/wt.cu:170-172): the arithmetic is that of its column passes (separable.cu:135-176 analysis,
// :250-326 synthesis) with a whole plane of P = Nr * Nc samples in the place of a row.
//
//   dwt3_depth_fwd   in [Nz][P]  ->  out [2 * div2(Nz)][P]: the low-pass slices, then the high-pass slices, back to back
//   dwt3_depth_inv   in [2 * Nin][P] (low slices, high slices)  ->  out [Nz][P], Nz = 2 Nin or 2 Nin - 1 (the virtual
//                    last slice of an odd depth is dropped, separable.cu:296)
//
// Pure streaming: a thread owns VEC neighbouring columns of the plane (VEC * sizeof(real_t) = 16 B where every slice starts
// on a 16-B boundary -- P a multiple of VEC --, else one column: a dword per lane, 256 B per wave instruction) and WALKS a
// segment of output slices.  The filter's history -- HLEN input slices forward, HLEN / 2 slices of each half-band inverse --
// stays in registers; a step shifts it and loads two new slices, which are fetched one step ahead of their use.  Nothing is
// shared between threads: no LDS, no barrier.  gridDim.x = column groups, gridDim.y = depth segments; a segment re-reads its
// history (HLEN - 2 slices).  Long filters (18-40 taps) take fewer columns per thread so that the window fits the registers.
//
// Every source index is periodised into [0, Nz) (forward) or [0, Nin) (inverse) by an incrementing counter that wraps, so a
// depth shorter than the filter wraps as often as it must and no access can leave the input; stores go to output slices
// 0 .. extent - 1 only and to columns < P only.
//
// The index math below is plain inline functions; with -DPDWT_CPU_EMU the tile functions run on the host
// (tests/cpu_emu/emu_axis.cpp).
#pragma once

#include "axis_common.hpp"
#include "strip_walk.hpp"

namespace pdwt {

struct Dwt3Args {
    const real_t* in;
    real_t* out;
    int Nz;       // depth of the signal domain: the forward's input, the inverse's output
    int Nh;       // div2(Nz): slices per half-band
    long long P;  // samples per slice
    int seg;      // steps per depth segment (>= 1)
    FilterBank fb;  // forward: dec_lo, dec_hi; inverse: rec_lo, rec_hi
};

// ---- index math (host and device) -------------------------------------------------------------------------------------

PDWT_HD int dwt3_div2(int n) { return (n + (n & 1)) / 2; }

// steps of a whole walk: forward, one per output slice pair (low k, high k); inverse, one per pair of output slices that
// share their sources -- q = (g + shift) / 2 for output slice g
PDWT_HD int dwt3_inv_shift(int hlen) { return ((hlen / 2) & 1) ? 0 : 1; }  // pdwt_oracle.c: syn_params
PDWT_HD int dwt3_fwd_steps(int Nz) { return dwt3_div2(Nz); }
PDWT_HD int dwt3_inv_steps(int Nz, int hlen) { return (Nz - 1 + dwt3_inv_shift(hlen)) / 2 + 1; }

PDWT_HD int dwt3_true_mod(int i, int n) {
    const int m = i % n;
    return m < 0 ? m + n : m;
}

// forward: position in the extended period (Nz + (Nz odd) slices) of the FIRST tap's source of output slice k
PDWT_HD int dwt3_fwd_first(int k, int hlen, int Nz) {
    const int c = (hlen & 1) ? hlen / 2 : hlen / 2 - 1;
    return dwt3_true_mod(2 * k - c, Nz + (Nz & 1));
}
// the next position, and the slice a position reads (the virtual slice of an odd depth repeats the last one)
PDWT_HD int dwt3_next(int pos, int period) { return pos + 1 == period ? 0 : pos + 1; }
PDWT_HD int dwt3_fwd_slice(int pos, int Nz) { return pos >= Nz ? Nz - 1 : pos; }

// inverse: first source slice (of both half-bands) of step q; output slices of step q and the taps they use:
//   g0 = 2 q - shift      taps hlen - 2 - 2 j   (j = 0 .. hlen / 2 - 1 over consecutive sources)
//   g1 = 2 q + 1 - shift  taps hlen - 1 - 2 j
PDWT_HD int dwt3_inv_first(int q, int hlen, int Nin) { return dwt3_true_mod(q - (hlen / 2) / 2, Nin); }
PDWT_HD int dwt3_inv_out0(int q, int hlen) { return 2 * q - dwt3_inv_shift(hlen); }

// Launch geometry, shared by the launchers (launch_depth3.hip) and the emulation (tests/cpu_emu/emu_axis.cpp).  Columns per thread
// of the wide path: 16 B per lane up to 16 taps, 8 B from 18 taps on (axis_common.hpp: axis_width picks it or 1 for a launch).
constexpr int dwt3_wide(int hlen) { return (int)(16 / sizeof(real_t)) / (hlen > 16 ? 2 : 1); }
// the shared geometry under this family's names, as the emulation spells it
constexpr int kDwt3NT = kAxisNT;
static inline int dwt3_width(const void* in, const void* out, long long P, int hlen) { return axis_width(in, out, P, dwt3_wide(hlen)); }
static inline long long dwt3_col_groups(long long P, int width) { return axis_col_groups(P, width); }

// Steps per segment: the walk of a workgroup re-reads `warm` steps' worth of history, so long segments are cheaper, but the
// chip wants `slots` resident workgroups (strip_walk.hpp: the fewest rounds x steps per workgroup).
static inline int dwt3_pick_seg(int steps, long long col_groups, int hlen, int slots) {
    const int warm = hlen / 2 - 1;
    return strip_walk_seg(steps, col_groups, 1, warm, slots > 0 ? slots : 1);
}

// ---- forward ------------------------------------------------------------------------------------------------------------
// out[k] = sum_j in[per(2 k - c + j)] * f[HLEN - 1 - j]   (separable.cu:135-176)

template <int HLEN, int VEC, int NT>
PDWT_DEVICE void dwt3_depth_fwd_tile(const Dwt3Args& a, const real_t* PDWT_RESTRICT flo, const real_t* PDWT_RESTRICT fhi, long long bx, int by) {
    PDWT_FOR_THREADS(tid, NT) {
        const long long col = (bx * NT + tid) * VEC;
        const int k0 = by * a.seg;
        if (col < a.P && k0 < a.Nh) {
            const int k1 = k0 + a.seg < a.Nh ? k0 + a.seg : a.Nh;
            const int period = a.Nz + (a.Nz & 1);
            int pos = dwt3_fwd_first(k0, HLEN, a.Nz);
            AxisVec<VEC> w[HLEN];
#pragma unroll
            for (int j = 0; j < HLEN; j++) {
                w[j] = axis_load<VEC>(a.in, dwt3_fwd_slice(pos, a.Nz), a.P, col);
                pos = dwt3_next(pos, period);
            }
            for (int k = k0; k < k1; k++) {
                // the two slices of the next step (periodised: always inside the input, also behind the last step)
                const AxisVec<VEC> n0 = axis_load<VEC>(a.in, dwt3_fwd_slice(pos, a.Nz), a.P, col);
                pos = dwt3_next(pos, period);
                const AxisVec<VEC> n1 = axis_load<VEC>(a.in, dwt3_fwd_slice(pos, a.Nz), a.P, col);
                pos = dwt3_next(pos, period);
                AxisVec<VEC> lo, hi;
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    real_t aL = 0, aH = 0;
#pragma unroll
                    for (int j = 0; j < HLEN; j++) {
                        aL = pdwt_fma(w[j].v[v], flo[HLEN - 1 - j], aL);
                        aH = pdwt_fma(w[j].v[v], fhi[HLEN - 1 - j], aH);
                    }
                    lo.v[v] = aL;
                    hi.v[v] = aH;
                }
                axis_store<VEC>(a.out, k, a.P, col, lo);
                axis_store<VEC>(a.out, (long long)a.Nh + k, a.P, col, hi);
#pragma unroll
                for (int j = 0; j + 2 < HLEN; j++) w[j] = w[j + 2];
                if (HLEN >= 2) {
                    w[HLEN - 2] = n0;
                    w[HLEN - 1] = n1;
                }
            }
        }
    }
}

// ---- inverse ------------------------------------------------------------------------------------------------------------
// out[g] = sum_j lowband[(q - c + j) mod Nin] * rlo[t_j] + highband[...] * rhi[t_j],  q = (g + shift) / 2   (pdwt_oracle.c:142-175)

template <int HLEN, int VEC, int NT>
PDWT_DEVICE void dwt3_depth_inv_tile(const Dwt3Args& a, const real_t* PDWT_RESTRICT flo, const real_t* PDWT_RESTRICT fhi, long long bx, int by) {
    constexpr int H2 = HLEN / 2;
    PDWT_FOR_THREADS(tid, NT) {
        const long long col = (bx * NT + tid) * VEC;
        const int steps = dwt3_inv_steps(a.Nz, HLEN);
        const int q0 = by * a.seg;
        if (col < a.P && q0 < steps) {
            const int q1 = q0 + a.seg < steps ? q0 + a.seg : steps;
            const int Nin = a.Nh;
            int pos = dwt3_inv_first(q0, HLEN, Nin);
            AxisVec<VEC> wa[H2], wd[H2];
#pragma unroll
            for (int j = 0; j < H2; j++) {
                wa[j] = axis_load<VEC>(a.in, pos, a.P, col);
                wd[j] = axis_load<VEC>(a.in, (long long)Nin + pos, a.P, col);
                pos = dwt3_next(pos, Nin);
            }
            for (int q = q0; q < q1; q++) {
                const AxisVec<VEC> na = axis_load<VEC>(a.in, pos, a.P, col);
                const AxisVec<VEC> nd = axis_load<VEC>(a.in, (long long)Nin + pos, a.P, col);
                pos = dwt3_next(pos, Nin);
                AxisVec<VEC> o0, o1;
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    real_t ra0 = 0, rd0 = 0, ra1 = 0, rd1 = 0;
#pragma unroll
                    for (int j = 0; j < H2; j++) {
                        ra0 = pdwt_fma(wa[j].v[v], flo[HLEN - 2 - 2 * j], ra0);
                        rd0 = pdwt_fma(wd[j].v[v], fhi[HLEN - 2 - 2 * j], rd0);
                        ra1 = pdwt_fma(wa[j].v[v], flo[HLEN - 1 - 2 * j], ra1);
                        rd1 = pdwt_fma(wd[j].v[v], fhi[HLEN - 1 - 2 * j], rd1);
                    }
                    o0.v[v] = ra0 + rd0;
                    o1.v[v] = ra1 + rd1;
                }
                const int g0 = dwt3_inv_out0(q, HLEN);
                if (g0 >= 0 && g0 < a.Nz) axis_store<VEC>(a.out, g0, a.P, col, o0);
                if (g0 + 1 < a.Nz) axis_store<VEC>(a.out, g0 + 1, a.P, col, o1);
#pragma unroll
                for (int j = 0; j + 1 < H2; j++) {
                    wa[j] = wa[j + 1];
                    wd[j] = wd[j + 1];
                }
                wa[H2 - 1] = na;
                wd[H2 - 1] = nd;
            }
        }
    }
}

#ifndef PDWT_CPU_EMU
// Where the taps live.  Up to 16 taps: in the kernel-argument segment, fetched with scalar loads into SGPRs (at most 32 of them).
// From 18 taps on the 2 x HLEN taps (fp64: twice the dwords) do not fit the scalar register file -- hipcc spills SGPRs into VGPR
// lanes and reads them back inside the FMA loop --, so the workgroup stages them in LDS once (as dwt2_long_kernels.hpp keeps its
// tap tables out of the scalar file) and the FMA loop reads them from there with uniform addresses.
template <int HLEN, int VEC, bool INV>
PDWT_DEVICE void dwt3_depth_run(const Dwt3Args& a) {
    if constexpr (HLEN >= kAxisTapsInLds) {
        __shared__ real_t taps[2 * HLEN];
        if (threadIdx.x < HLEN) taps[threadIdx.x] = a.fb.lo[threadIdx.x];
        else if (threadIdx.x < 2 * HLEN) taps[threadIdx.x] = a.fb.hi[threadIdx.x - HLEN];
        __syncthreads();
        if constexpr (INV) dwt3_depth_inv_tile<HLEN, VEC, kAxisNT>(a, taps, taps + HLEN, (long long)blockIdx.x, (int)blockIdx.y);
        else dwt3_depth_fwd_tile<HLEN, VEC, kAxisNT>(a, taps, taps + HLEN, (long long)blockIdx.x, (int)blockIdx.y);
    } else {
        if constexpr (INV) dwt3_depth_inv_tile<HLEN, VEC, kAxisNT>(a, a.fb.lo, a.fb.hi, (long long)blockIdx.x, (int)blockIdx.y);
        else dwt3_depth_fwd_tile<HLEN, VEC, kAxisNT>(a, a.fb.lo, a.fb.hi, (long long)blockIdx.x, (int)blockIdx.y);
    }
}

template <int HLEN, int VEC>
__global__ __launch_bounds__(kAxisNT) void dwt3_depth_fwd_kernel(const Dwt3Args a) {
    dwt3_depth_run<HLEN, VEC, false>(a);
}

template <int HLEN, int VEC>
__global__ __launch_bounds__(kAxisNT) void dwt3_depth_inv_kernel(const Dwt3Args a) {
    dwt3_depth_run<HLEN, VEC, true>(a);
}
#endif

}  // namespace pdwt
