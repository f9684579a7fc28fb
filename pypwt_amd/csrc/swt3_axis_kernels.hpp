// swt3_axis_kernels.hpp -- one UNDECIMATED (a-trous) wavelet level along the SLOWEST axis of a volume: the depth pass of a
// stationary pdwt_volume (volume.cpp, do_swt = 1).  The reference has no 3D transform; the arithmetic is that of its SWT column
// passes (pdwt_oracle.c:199-277) with a whole plane of P = Nr * Nc samples in the place of a row, dilation f = 2^(level - 1).
//
//   swt3_depth_fwd   in [Nz][P]    ->  out [2 Nz][P]: the Nz low slices, then the Nz high slices          c = HLEN / 2 - 1
//                        lo[g] = sum_j in[(g + (j - c) f) mod Nz] * dec_lo[HLEN - 1 - j]        (hi likewise with dec_hi)
//   swt3_depth_inv   in [2 Nz][P]  ->  out [Nz][P]                                                        c = HLEN / 2
//                        out[g] = 1/2 sum_j (lo[(g + (j - c) f) mod Nz] * rec_lo[HLEN - 1 - j] + hi[same] * rec_hi[HLEN - 1 - j])
//
// The access shape is dwt3_axis_kernels.hpp's: a thread owns VEC neighbouring columns of the plane (16 B per lane where the
// register window allows it and every slice starts on such a boundary, else narrower, down to one column), nothing is shared
// between threads: no LDS for data, no barrier.  The WALK differs.  A thread steps along an orbit of g -> (g + f) mod Nz: there are
// gcd(f, Nz) orbits of Nz / gcd outputs each (for f | Nz the f residue classes), and along an orbit the filter window shifts by
// ONE slot per step.  So a step loads one new slice (the inverse: one of each half-band) and stores two (the inverse: one); the
// window of HLEN slices (2 HLEN in the inverse) stays in registers.  A forward pass reads about one volume and writes two, where
// a gather would read HLEN volumes.  gridDim.x = column groups, gridDim.y = orbits x segments of an orbit; a segment re-reads
// its history (HLEN - 1 slices).
//
// Every source index is periodised into [0, Nz) by a counter that adds (f mod Nz) and wraps; the first index of a segment is a
// true modulo (c f may exceed Nz many times over).  Nothing is read outside the input, and stores go to slices 0 .. extent - 1
// and columns < P only, for any Nz >= 1, f >= 1 and P >= 1.
//
// The index math below is plain inline functions; with -DPDWT_CPU_EMU the tile functions run on the host
// (tests/cpu_emu/emu_swt_axis.cpp).
#pragma once

#include "axis_common.hpp"
#include "strip_walk.hpp"

namespace pdwt {

struct Swt3Args {
    const real_t* in;
    real_t* out;
    int Nz;         // slices of the signal domain (every band has as many)
    int fm;         // f mod Nz: what a step adds to a slice index
    int orbits;     // gcd(f, Nz)
    int steps;      // Nz / orbits: outputs of one orbit
    int seg;        // steps per segment (>= 1)
    int nseg;       // ceil(steps / seg): blockIdx.y = orbit * nseg + segment
    long long P;    // samples per slice
    FilterBank fb;  // forward: dec_lo, dec_hi; inverse: rec_lo, rec_hi
};

// ---- index math (host and device) -------------------------------------------------------------------------------------

PDWT_HD int swt3_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}
PDWT_HD int swt3_orbits(int f, int Nz) { return swt3_gcd(f % Nz, Nz); }  // gcd(0, Nz) = Nz: Nz | f, every slice its own orbit
PDWT_HD int swt3_steps(int f, int Nz) { return Nz / swt3_orbits(f, Nz); }
PDWT_HD int swt3_centre(int hlen, bool inverse) { return inverse ? hlen / 2 : hlen / 2 - 1; }

// output slice of step t of orbit o, and the first tap's source slice of an output slice g: true modulos, once per segment
PDWT_HD int swt3_out_slice(int o, int t, int fm, int Nz) { return (int)(((long long)o + (long long)t * fm) % Nz); }
PDWT_HD int swt3_first_src(int g, int c, int fm, int Nz) {
    const long long m = ((long long)g - (long long)c * fm) % Nz;
    return (int)(m < 0 ? m + Nz : m);
}
// the next slice along the orbit (fm < Nz: one conditional subtraction)
PDWT_HD int swt3_next(int pos, int fm, int Nz) {
    const int n = pos + fm;
    return n >= Nz ? n - Nz : n;
}

// Launch geometry, shared by the launchers (launch_depth3.hip) and the emulation (tests/cpu_emu/emu_swt_axis.cpp).  Columns per
// thread of the wide path: the register window is HLEN x VEC values forward and 2 HLEN x VEC inverse, so 16 B per lane up to 16
// taps forward (8 inverse), half of that up to 40 (16 inverse), and a quarter for the inverse from 18 taps on -- never below one
// column (fp64 reaches it earlier).  tools/spillscan.py confirms that no instantiation spills; docs/KERNELS.md has the counts.
constexpr int swt3_wide(int hlen, bool inverse) {
    const int full = (int)(16 / sizeof(real_t));
    const int div = inverse ? (hlen > 16 ? 4 : hlen > 8 ? 2 : 1) : (hlen > 16 ? 2 : 1);
    return full / div > 1 ? full / div : 1;
}

// Steps per segment of an orbit walk: a segment re-reads HLEN - 1 slices of history, the chip wants `slots` resident workgroups,
// and the orbits are independent units beside the column groups (strip_walk.hpp: the fewest rounds x steps per workgroup).
// the shared geometry under this family's names, as the emulation spells it
constexpr int kSwt3NT = kAxisNT;
static inline int swt3_width(const void* in, const void* out, long long P, int hlen, bool inverse) { return axis_width(in, out, P, swt3_wide(hlen, inverse)); }
static inline long long swt3_col_groups(long long P, int width) { return axis_col_groups(P, width); }

static inline int swt3_pick_seg(int steps, long long col_groups, int orbits, int hlen, int slots) {
    return strip_walk_seg(steps, col_groups * orbits, 1, hlen - 1, slots > 0 ? slots : 1);
}

// the geometry of one pass; seg <= 0 or beyond the walk: one segment per orbit
static inline void swt3_geometry(Swt3Args& a, int Nz, int f, int seg) {
    a.Nz = Nz;
    a.fm = f % Nz;
    a.orbits = swt3_orbits(f, Nz);
    a.steps = Nz / a.orbits;
    a.seg = seg < 1 || seg > a.steps ? a.steps : seg;
    a.nseg = (a.steps + a.seg - 1) / a.seg;
}

// ---- forward ------------------------------------------------------------------------------------------------------------

template <int HLEN, int VEC, int NT>
PDWT_DEVICE void swt3_depth_fwd_tile(const Swt3Args& a, const real_t* PDWT_RESTRICT flo, const real_t* PDWT_RESTRICT fhi, long long bx, int by) {
    PDWT_FOR_THREADS(tid, NT) {
        const long long col = (bx * NT + tid) * VEC;
        const int o = by / a.nseg, t0 = (by - o * a.nseg) * a.seg;
        if (col < a.P && o < a.orbits && t0 < a.steps) {
            const int t1 = t0 + a.seg < a.steps ? t0 + a.seg : a.steps;
            int g = swt3_out_slice(o, t0, a.fm, a.Nz);
            int pos = swt3_first_src(g, swt3_centre(HLEN, false), a.fm, a.Nz);
            AxisVec<VEC> w[HLEN];
#pragma unroll
            for (int j = 0; j < HLEN; j++) {
                w[j] = axis_load<VEC>(a.in, pos, a.P, col);
                pos = swt3_next(pos, a.fm, a.Nz);
            }
            for (int t = t0; t < t1; t++) {
                // the slice of the next step (periodised: always inside the input, also behind the last step)
                const AxisVec<VEC> n0 = axis_load<VEC>(a.in, pos, a.P, col);
                pos = swt3_next(pos, a.fm, a.Nz);
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
                axis_store<VEC>(a.out, g, a.P, col, lo);
                axis_store<VEC>(a.out, (long long)a.Nz + g, a.P, col, hi);
                g = swt3_next(g, a.fm, a.Nz);
#pragma unroll
                for (int j = 0; j + 1 < HLEN; j++) w[j] = w[j + 1];
                w[HLEN - 1] = n0;
            }
        }
    }
}

// ---- inverse ------------------------------------------------------------------------------------------------------------

template <int HLEN, int VEC, int NT>
PDWT_DEVICE void swt3_depth_inv_tile(const Swt3Args& a, const real_t* PDWT_RESTRICT flo, const real_t* PDWT_RESTRICT fhi, long long bx, int by) {
    PDWT_FOR_THREADS(tid, NT) {
        const long long col = (bx * NT + tid) * VEC;
        const int o = by / a.nseg, t0 = (by - o * a.nseg) * a.seg;
        if (col < a.P && o < a.orbits && t0 < a.steps) {
            const int t1 = t0 + a.seg < a.steps ? t0 + a.seg : a.steps;
            int g = swt3_out_slice(o, t0, a.fm, a.Nz);
            int pos = swt3_first_src(g, swt3_centre(HLEN, true), a.fm, a.Nz);
            AxisVec<VEC> wa[HLEN], wd[HLEN];
#pragma unroll
            for (int j = 0; j < HLEN; j++) {
                wa[j] = axis_load<VEC>(a.in, pos, a.P, col);
                wd[j] = axis_load<VEC>(a.in, (long long)a.Nz + pos, a.P, col);
                pos = swt3_next(pos, a.fm, a.Nz);
            }
            for (int t = t0; t < t1; t++) {
                const AxisVec<VEC> na = axis_load<VEC>(a.in, pos, a.P, col);
                const AxisVec<VEC> nd = axis_load<VEC>(a.in, (long long)a.Nz + pos, a.P, col);
                pos = swt3_next(pos, a.fm, a.Nz);
                AxisVec<VEC> r;
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    real_t ra = 0, rd = 0;
#pragma unroll
                    for (int j = 0; j < HLEN; j++) {
                        ra = pdwt_fma(wa[j].v[v], flo[HLEN - 1 - j], ra);
                        rd = pdwt_fma(wd[j].v[v], fhi[HLEN - 1 - j], rd);
                    }
                    r.v[v] = (real_t)0.5 * (ra + rd);
                }
                axis_store<VEC>(a.out, g, a.P, col, r);
                g = swt3_next(g, a.fm, a.Nz);
#pragma unroll
                for (int j = 0; j + 1 < HLEN; j++) {
                    wa[j] = wa[j + 1];
                    wd[j] = wd[j + 1];
                }
                wa[HLEN - 1] = na;
                wd[HLEN - 1] = nd;
            }
        }
    }
}

#ifndef PDWT_CPU_EMU
// Where the taps live: dwt3_axis_kernels.hpp, dwt3_depth_run -- up to 16 taps in the kernel-argument segment (scalar loads), from
// 18 taps on staged in LDS once per workgroup and read with uniform addresses.
template <int HLEN, int VEC, bool INV>
PDWT_DEVICE void swt3_depth_run(const Swt3Args& a) {
    if constexpr (HLEN >= kAxisTapsInLds) {
        __shared__ real_t taps[2 * HLEN];
        if (threadIdx.x < HLEN) taps[threadIdx.x] = a.fb.lo[threadIdx.x];
        else if (threadIdx.x < 2 * HLEN) taps[threadIdx.x] = a.fb.hi[threadIdx.x - HLEN];
        __syncthreads();
        if constexpr (INV) swt3_depth_inv_tile<HLEN, VEC, kAxisNT>(a, taps, taps + HLEN, (long long)blockIdx.x, (int)blockIdx.y);
        else swt3_depth_fwd_tile<HLEN, VEC, kAxisNT>(a, taps, taps + HLEN, (long long)blockIdx.x, (int)blockIdx.y);
    } else {
        if constexpr (INV) swt3_depth_inv_tile<HLEN, VEC, kAxisNT>(a, a.fb.lo, a.fb.hi, (long long)blockIdx.x, (int)blockIdx.y);
        else swt3_depth_fwd_tile<HLEN, VEC, kAxisNT>(a, a.fb.lo, a.fb.hi, (long long)blockIdx.x, (int)blockIdx.y);
    }
}

template <int HLEN, int VEC>
__global__ __launch_bounds__(kAxisNT) void swt3_depth_fwd_kernel(const Swt3Args a) {
    swt3_depth_run<HLEN, VEC, false>(a);
}

template <int HLEN, int VEC>
__global__ __launch_bounds__(kAxisNT) void swt3_depth_inv_kernel(const Swt3Args a) {
    swt3_depth_run<HLEN, VEC, true>(a);
}
#endif

}  // namespace pdwt
