// volume_shift_kernels.hpp -- circular shifts of a volume [Nz][Nr][Nc] (pdwt_volume_circshift, the cycle spinning of
// pdwt_volume_forward / pdwt_volume_inverse and pdwt_volume_cycle_spin_async of include/pypwt_amd.h; gfx950).
//
//   vol_circshift_kernel     out[z][r][c] = in[z - sz][r - sr][c - sc], every index modulo its size: numpy.roll(in, (sz, sr, sc)),
//                            the sense of the 2D circshift_kernel (ops_kernels.hpp) on rows and columns and the same on depth;
//   vol_unshift_acc_kernel   acc[p] = (first ? 0 : acc[p]) + w rec[p + s]: the shift BACK of one reconstruction, weighted and added
//                            to the running mean of the cycle spinning.  It is the same walk with the shift (N - s) mod N.
//
// Both take shifts already reduced to 0 .. N - 1 (vol_shift_reduce, on the host).  Pure data movement, out of place, no LDS:
//   - the volume is cut into PIECES: a piece is up to 256 consecutive columns of ONE output row (z, r).  z and r are wrapped once
//     per piece, which gives one source row; only the column is wrapped per access, and it splits the piece into at most two
//     contiguous runs (output columns below sc come from the end of the source row, the others from its start);
//   - a wavefront moves kVolShiftUnroll consecutive pieces per trip: the piece -> (z, r, segment) division is done once per trip,
//     the next pieces follow by counting, and the loads of all of them are issued before the first store;
//   - mode 2 (Nc % 4 == 0, sc % 4 == 0, both buffers aligned): a lane moves one 16-B (fp64: 32-B) group per piece;
//     mode 1 (Nc % 4 == 0, the output aligned): the same group is STORED whole but loaded as four values -- the source of a group
//             is not aligned, and a group may straddle the column wrap;
//     mode 0 (anything else): value by value, lane l of a piece takes columns l, l + 64, ..: every access of the wavefront is
//             one contiguous run (two at the wrap).
//
// The index math is plain inline code that also compiles with g++ -DPDWT_CPU_EMU (tests/cpu_emu/emu_volume_shift.cpp walks every
// wavefront of both kernels with vol_shift_wave, the function the kernels walk with); the kernels are thin wrappers.
#pragma once

#include <stdint.h>

#include "kernels_common.hpp"

#ifndef PDWT_HOST_DEVICE
#ifdef PDWT_CPU_EMU
#define PDWT_HOST_DEVICE inline
#else
#define PDWT_HOST_DEVICE __host__ __device__ __forceinline__
#endif
#endif

namespace pdwt {

constexpr int kVolShiftThreads = 256;
constexpr int kVolShiftWaves = kVolShiftThreads / 64;
constexpr int kVolShiftSeg = 256;     // columns of a piece: one group of four per lane of a wavefront
constexpr int kVolShiftUnroll = 4;    // pieces per wavefront and trip
constexpr int kVolShiftMaxGrid = 2048;

// Passed by value in the kernel-argument segment.  Shifts are reduced: 0 <= s < N.
struct VolShiftGeom {
    int Nz, Nr, Nc;
    int sz, sr, sc;
    int segs;          // pieces per row
    int mode;          // 0 values, 1 group stores and value loads, 2 groups
    long long pieces;  // Nz Nr segs
    long long trips;   // wavefront trips: ceil(pieces / kVolShiftUnroll)
};

// a caller's shift, of any sign and size, as 0 .. n - 1
PDWT_HOST_DEVICE int vol_shift_reduce(long long s, int n) {
    const long long m = s % n;
    return (int)(m < 0 ? m + n : m);
}
// the reduced shift that undoes the reduced shift s
PDWT_HOST_DEVICE int vol_shift_inverse(int s, int n) { return s ? n - s : 0; }
// the source index of output index i along an axis of n samples shifted by the reduced s
PDWT_HOST_DEVICE int vol_shift_src(int i, int s, int n) {
    const int j = i - s;
    return j < 0 ? j + n : j;
}

// The geometry of one launch: (sz, sr, sc) reduced; src / dst only decide the access width.  No HIP call.
inline VolShiftGeom vol_shift_geom(int Nz, int Nr, int Nc, int sz, int sr, int sc, const void* src, const void* dst) {
    VolShiftGeom g;
    g.Nz = Nz, g.Nr = Nr, g.Nc = Nc;
    g.sz = sz, g.sr = sr, g.sc = sc;
    g.segs = (Nc + kVolShiftSeg - 1) / kVolShiftSeg;
    const uintptr_t group = 4 * sizeof(real_t);
    const bool wide_out = (Nc & 3) == 0 && reinterpret_cast<uintptr_t>(dst) % group == 0;
    const bool wide_in = wide_out && (sc & 3) == 0 && reinterpret_cast<uintptr_t>(src) % group == 0;
    g.mode = wide_in ? 2 : (wide_out ? 1 : 0);
    g.pieces = (long long)Nz * Nr * g.segs;
    g.trips = (g.pieces + kVolShiftUnroll - 1) / kVolShiftUnroll;
    return g;
}
// The same from a caller's shifts, of any sign and size: reduced, and with `back` replaced by the shifts that undo them.
inline VolShiftGeom vol_shift_geom_of(int Nz, int Nr, int Nc, long long sz, long long sr, long long sc, bool back, const void* src,
                                      const void* dst) {
    int z = vol_shift_reduce(sz, Nz), r = vol_shift_reduce(sr, Nr), c = vol_shift_reduce(sc, Nc);
    if (back) z = vol_shift_inverse(z, Nz), r = vol_shift_inverse(r, Nr), c = vol_shift_inverse(c, Nc);
    return vol_shift_geom(Nz, Nr, Nc, z, r, c, src, dst);
}
// workgroups of the launch: the wavefronts stride over the trips
inline int vol_shift_grid(const VolShiftGeom& g, int max_grid = kVolShiftMaxGrid) {
    const long long wgs = (g.trips + kVolShiftWaves - 1) / kVolShiftWaves;
    return (int)(wgs < max_grid ? wgs : max_grid);
}

// piece -> output row (z, r) and column segment
PDWT_HOST_DEVICE void vol_shift_piece(const VolShiftGeom& g, long long piece, int* z, int* r, int* seg) {
    const long long row = piece / g.segs;
    *seg = (int)(piece - row * g.segs);
    *z = (int)(row / g.Nr);
    *r = (int)(row - (long long)*z * g.Nr);
}
// the piece behind (z, r, seg), by counting
PDWT_HOST_DEVICE void vol_shift_next(const VolShiftGeom& g, int* z, int* r, int* seg) {
    if (++*seg < g.segs) return;
    *seg = 0;
    if (++*r < g.Nr) return;
    *r = 0;
    ++*z;
}
// first element of output row (z, r), and of the source row it is read from: z and r are wrapped here, once per piece
PDWT_HOST_DEVICE long long vol_shift_dst_row(const VolShiftGeom& g, int z, int r) { return ((long long)z * g.Nr + r) * g.Nc; }
PDWT_HOST_DEVICE long long vol_shift_src_row(const VolShiftGeom& g, int z, int r) {
    return ((long long)vol_shift_src(z, g.sz, g.Nz) * g.Nr + vol_shift_src(r, g.sr, g.Nr)) * g.Nc;
}
// The two runs of output columns [c0, c1): [c0, *m) reads source columns c + Nc - sc, [*m, c1) reads c - sc.
PDWT_HOST_DEVICE void vol_shift_runs(const VolShiftGeom& g, int c0, int c1, int* m) { *m = g.sc < c0 ? c0 : (g.sc > c1 ? c1 : g.sc); }
// the source column of output column c
PDWT_HOST_DEVICE int vol_shift_col(const VolShiftGeom& g, int c) { return vol_shift_src(c, g.sc, g.Nc); }

// Lane `lane` of the wavefront that makes trip `trip`: its share of the kVolShiftUnroll pieces of the trip.
//   ld1(src element) -> value, ld4(src element) -> group;  st1(dst element, value), st4(dst element, group).
// MODE is g.mode.  Every load of a trip (mode 0: of a piece) is issued before its first store.
template <int MODE, typename L1, typename L4, typename S1, typename S4>
PDWT_DEVICE void vol_shift_wave(const VolShiftGeom& g, long long trip, int lane, L1 ld1, L4 ld4, S1 st1, S4 st4) {
    const long long piece = trip * kVolShiftUnroll;
    int z, r, seg;
    vol_shift_piece(g, piece, &z, &r, &seg);
    if (MODE == 0) {
        for (int u = 0; u < kVolShiftUnroll && piece + u < g.pieces; u++) {
            const long long dst = vol_shift_dst_row(g, z, r), src = vol_shift_src_row(g, z, r);
            const int c0 = seg * kVolShiftSeg, c1 = c0 + kVolShiftSeg < g.Nc ? c0 + kVolShiftSeg : g.Nc;
            real_t v[kVolShiftSeg / 64];
#pragma unroll
            for (int j = 0; j < kVolShiftSeg / 64; j++) {
                const int c = c0 + lane + 64 * j;
                if (c < c1) v[j] = ld1(src + vol_shift_col(g, c));
            }
#pragma unroll
            for (int j = 0; j < kVolShiftSeg / 64; j++) {
                const int c = c0 + lane + 64 * j;
                if (c < c1) st1(dst + c, v[j]);
            }
            vol_shift_next(g, &z, &r, &seg);
        }
    } else {
        real4_t v[kVolShiftUnroll];
        long long at[kVolShiftUnroll];  // the lane's destination group of piece u, or -1: none
#pragma unroll
        for (int u = 0; u < kVolShiftUnroll; u++) {
            const int c = seg * kVolShiftSeg + 4 * lane;
            at[u] = -1;
            if (piece + u < g.pieces && c < g.Nc) {
                const long long src = vol_shift_src_row(g, z, r);
                at[u] = vol_shift_dst_row(g, z, r) + c;
                if (MODE == 2) {
                    v[u] = ld4(src + vol_shift_col(g, c));
                } else {
                    v[u].x = ld1(src + vol_shift_col(g, c));
                    v[u].y = ld1(src + vol_shift_col(g, c + 1));
                    v[u].z = ld1(src + vol_shift_col(g, c + 2));
                    v[u].w = ld1(src + vol_shift_col(g, c + 3));
                }
            }
            vol_shift_next(g, &z, &r, &seg);
        }
#pragma unroll
        for (int u = 0; u < kVolShiftUnroll; u++)
            if (at[u] >= 0) st4(at[u], v[u]);
    }
}

// the accumulate of the running mean: w x alone the first time (no memset of the accumulator), else acc + w x, one fused
// multiply-add on the GPU
PDWT_DEVICE real_t vol_acc(real_t acc, real_t w, real_t x, int first) { return first ? w * x : pdwt_fma(w, x, acc); }

#if !defined(PDWT_CPU_EMU) && !defined(PDWT_INLINE_HELPERS_ONLY)

// out = circshift(in) by g's reduced shifts; grid = vol_shift_grid(g), 256 threads; `in` and `out` never overlap
template <int MODE>
__global__ void __launch_bounds__(kVolShiftThreads) vol_circshift_kernel(const real_t* __restrict__ in, real_t* __restrict__ out, VolShiftGeom g) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kVolShiftWaves;
    for (long long trip = (long long)blockIdx.x * kVolShiftWaves + (threadIdx.x >> 6); trip < g.trips; trip += waves)
        vol_shift_wave<MODE>(
            g, trip, lane, [&](long long i) { return in[i]; }, [&](long long i) { return *reinterpret_cast<const real4_t*>(in + i); },
            [&](long long i, real_t x) { out[i] = x; }, [&](long long i, const real4_t& x) { *reinterpret_cast<real4_t*>(out + i) = x; });
}

// acc = (first ? 0 : acc) + w circshift(rec) by g's reduced shifts (the caller passes the INVERSE of the shift that was applied);
// `acc` and `rec` never overlap
template <int MODE>
__global__ void __launch_bounds__(kVolShiftThreads) vol_unshift_acc_kernel(const real_t* __restrict__ rec, real_t* __restrict__ acc, VolShiftGeom g,
                                                                           real_t w, int first) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kVolShiftWaves;
    for (long long trip = (long long)blockIdx.x * kVolShiftWaves + (threadIdx.x >> 6); trip < g.trips; trip += waves)
        vol_shift_wave<MODE>(
            g, trip, lane, [&](long long i) { return rec[i]; }, [&](long long i) { return *reinterpret_cast<const real4_t*>(rec + i); },
            [&](long long i, real_t x) { acc[i] = vol_acc(first ? real_t(0) : acc[i], w, x, first); },
            [&](long long i, const real4_t& x) {
                real4_t a = x;
                if (first) {
                    a.x *= w, a.y *= w, a.z *= w, a.w *= w;
                } else {
                    const real4_t o = *reinterpret_cast<const real4_t*>(acc + i);
                    a.x = pdwt_fma(w, x.x, o.x), a.y = pdwt_fma(w, x.y, o.y), a.z = pdwt_fma(w, x.z, o.z), a.w = pdwt_fma(w, x.w, o.w);
                }
                *reinterpret_cast<real4_t*>(acc + i) = a;
            });
}

#endif  // !PDWT_CPU_EMU && !PDWT_INLINE_HELPERS_ONLY

}  // namespace pdwt
