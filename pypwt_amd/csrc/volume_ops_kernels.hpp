// volume_ops_kernels.hpp -- the per-sub-band and K-term operators of a volume (pdwt_volume_* of include/pypwt_amd.h; gfx950).
//
// A volume keeps its coefficients in the arenas of one batched 2D plan per level (volume.hpp): to such a plan an "image" is one
// slice, and the depth-low half of band A of every level below the last is an intermediate, not a coefficient.  The plans'
// own per-(band, image) operators therefore see slices; what pools them into the 1 + 7 L sub-bands of ONE volume is here:
//
//   vol_select_hist_kernel   the histogram pass of the rank select (select_kernels.hpp) over a table of contiguous RANGES, all
//                            levels in one launch, every piece into the volume's one histogram;
//   vol_keep_kernel          the keep sweep of the best K-term approximation over the same ranges;
//   vol_stats_reduce_kernel  the plans' per-slice sums added up per sub-band, one wavefront per sub-band, fixed order;
//   vol_norms_kernel         the sub-bands' sums added up, one wavefront, fixed order;
//   vol_table_kernel         BayesShrink / VisuShrink thresholds per sub-band, one thread each;
//   vol_expand_kernel        a table per sub-band written into every level plan's [4][2 div2(Nz)] table, one thread per entry,
//                            NaN (leave alone) for the intermediate halves;
//   vol_group_soft_kernel    the group soft threshold over the seven sub-bands of a position (and A_L), all levels in one launch,
//                            for the decimated and the stationary layout alike (VolGroupTable, further down);
//   vol_group_norm_kernel    the l2,1 norm of the same groups: one partial sum per workgroup, vol_group_norm_final_kernel adds them.
//
// A range is (arena base of its level's plan, first, end) in elements from that base: the sweeps align their 16-B (fp64: 32-B)
// groups by INDEX (ops_kernels.hpp: sweep_range), which is address alignment only because the base is the 256-B aligned arena;
// a depth half starts at div2(Nz) rows cols elements into its band, an odd number as often as not.
//
// The index math -- the range builder, the piece -> range map and the (level, band, slice) -> sub-band map -- is plain inline
// code that also compiles with g++ -DPDWT_CPU_EMU (tests/cpu_emu/emu_volume_ops.cpp); the kernels are thin wrappers.
#pragma once

#include <stdint.h>

#include "kernels_common.hpp"
#include "select_kernels.hpp"

// the sub-band numbering serves the host too (volume.cpp expands a host table with it)
#ifdef PDWT_CPU_EMU
#define PDWT_HOST_DEVICE inline
#else
#define PDWT_HOST_DEVICE __host__ __device__ __forceinline__
#endif

namespace pdwt {

// the level clamp leaves at most ilog2(65534) = 15 levels (volume.cpp: check_shape, clamp_levels)
constexpr int kVolMaxLevels = 16;
constexpr int kVolMaxRanges = 4 * kVolMaxLevels + 1;
constexpr int kVolKeepThreads = 256;

// The swept coefficients of a volume cut into workgroup-sized pieces of ONE range each; passed by value in the kernel-argument
// segment.  Range r is [first[r], end[r]) from base[r]; its pieces of `chunk` values are the workgroups blk[r] .. blk[r + 1] - 1.
// Per level: bands H, V, D whole and the depth-high half of band A; the LAST range is A_L (the depth-low half of band A of the
// last level), so that a sweep without the approximation is the same table launched with blk[nranges - 1] workgroups.
struct VolRangeTable {
    int nranges;
    long long chunk;
    real_t* base[kVolMaxRanges];
    long long first[kVolMaxRanges];
    long long end[kVolMaxRanges];
    int blk[kVolMaxRanges + 1];
};

// What the small kernels need to know of every level l (index l - 1): the slices per depth half, the elements of a sub-band, and
// the level plan's own slots (pdwt_adaptive_slots): sums [4][2 half][2], table [4][2 half].  entry[l - 1] = the first thread of
// vol_expand_kernel that writes level l's table.
struct VolLevels {
    int nlevels;
    int half[kVolMaxLevels];
    long long n[kVolMaxLevels];
    const double* stats[kVolMaxLevels];
    real_t* table[kVolMaxLevels];
    int entry[kVolMaxLevels + 1];
};

// pywt.wavedecn's sorted keys aad, ada, add, daa, dad, dda, ddd as (depth half, band of the level's 2D plan): k of (half, band)
PDWT_HOST_DEVICE int vol_key_index(int half, int band) {
    // half 0: A -, H ada 1, V aad 0, D add 2;  half 1: A daa 3, H dda 5, V dad 4, D ddd 6
    return half == 0 ? (band == 1 ? 1 : band == 2 ? 0 : 2) : (band == 0 ? 3 : band == 1 ? 5 : band == 2 ? 4 : 6);
}
// the (depth half, band) of key k, the other way round
PDWT_HOST_DEVICE void vol_key_place(int k, int* half, int* band) {
    *half = k >= 3;
    *band = k == 0 ? 2 : k == 1 ? 1 : k == 2 ? 3 : k == 3 ? 0 : k == 4 ? 2 : k == 5 ? 1 : 3;
}
// the sub-band `num` that slice `img` (0 .. 2 half - 1) of band `band` of level `level`'s plan belongs to; -1: the intermediate
// A_level of a level below the last
PDWT_HOST_DEVICE int vol_num_of(int level, int nlevels, int band, int img, int half) {
    const int hi = img >= half;
    if (band == 0 && !hi) return level == nlevels ? 0 : -1;
    return 1 + 7 * (level - 1) + vol_key_index(hi, band);
}
// where sub-band `num` lives: its level (1 .. L), depth half and band
PDWT_HOST_DEVICE void vol_locate(int num, int nlevels, int* level, int* half, int* band) {
    if (num == 0) {
        *level = nlevels;
        *half = 0;
        *band = 0;
        return;
    }
    *level = (num - 1) / 7 + 1;
    vol_key_place((num - 1) % 7, half, band);
}

// Appends level `level`'s ranges to `t` (call with level = 1 .. L in turn on a table whose nranges is 0, then vol_ranges_finish):
// off[b] = offset of band b in the plan's arena, half = slices per depth half, plane = values per slice.
inline void vol_ranges_add_level(VolRangeTable& t, real_t* arena, const long long off[4], int half, long long plane) {
    const long long n = (long long)half * plane;
    for (int b = 0; b < 4; b++) {
        const int r = t.nranges++;
        t.base[r] = arena;
        t.first[r] = off[b] + (b == 0 ? n : 0);
        t.end[r] = off[b] + 2 * n;
    }
}
// The last range, A_L, and the workgroup numbering: pieces of `chunk` values, at least `min_chunk` and about `target` of them
// over the whole table.  Returns the number of swept elements including A_L.
inline long long vol_ranges_finish(VolRangeTable& t, real_t* arena, long long off_a, int half, long long plane, long long target,
                                   long long min_chunk) {
    const int last = t.nranges++;
    t.base[last] = arena;
    t.first[last] = off_a;
    t.end[last] = off_a + (long long)half * plane;
    long long total = 0;
    for (int r = 0; r < t.nranges; r++) total += t.end[r] - t.first[r];
    long long chunk = ((total + target - 1) / target + 1023) / 1024 * 1024;
    if (chunk < min_chunk) chunk = min_chunk;
    t.chunk = chunk;
    long long blocks = 0;
    for (int r = 0; r < t.nranges; r++) {
        t.blk[r] = (int)blocks;
        blocks += (t.end[r] - t.first[r] + chunk - 1) / chunk;  // at most target + nranges in all
    }
    t.blk[t.nranges] = (int)blocks;
    return total;
}

// workgroup `blk`: its range and its piece [*a, *e) in elements from t.base[range]
PDWT_DEVICE int vol_piece(const VolRangeTable& t, int blk, long long* a, long long* e) {
    int r = 0;
    while (r + 1 < t.nranges && blk >= t.blk[r + 1]) r++;
    const long long lo = t.first[r] + (long long)(blk - t.blk[r]) * t.chunk;
    *a = lo;
    *e = lo + t.chunk < t.end[r] ? lo + t.chunk : t.end[r];
    return r;
}

// thread `idx` of vol_expand_kernel: its level (1 .. L), or 0 when idx is behind the last entry; *at = its entry [band][slice]
PDWT_DEVICE int vol_expand_entry(const VolLevels& v, int idx, int* at) {
    if (idx >= v.entry[v.nlevels]) return 0;
    int l = 1;
    while (l < v.nlevels && idx >= v.entry[l]) l++;
    *at = idx - v.entry[l - 1];
    return l;
}

// the keep sweep's arithmetic (keep_bands_kernel's): x stays, bit for bit, iff the bit pattern of |x| is at least k, else +0.0
PDWT_DEVICE real_t vol_keep(real_t x, select_key_t k) { return select_key(x) >= k ? x : real_t(0); }

// BayesShrink / VisuShrink threshold of a sub-band of n values out of its sum of squares and the noise level, in double (the
// arithmetic of denoise_table_kernel, ops_kernels.hpp); the caller rounds once
PDWT_DEVICE double vol_threshold(int method, double sumsq, long long n, double sigma, double visu) {
    if (method == 1) return sigma * visu;  // DENOISE_VISU
    const double var = sigma * sigma, eps = sizeof(real_t) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;
    const double d = sumsq / (double)n - var;
    return var / sqrt(d > eps ? d : eps);
}

// ---------------------------------------------------------------------------------------------------------------------
// The GROUP operators (group_soft_threshold, group_norm): the group at position i of level l is the seven detail sub-bands
// aad .. ddd at flat index i -- and A_L at the last level when asked for.  They live in the level's four band arrays [2 halves][n]:
// a depth-low member at band + i, a depth-high one at band + n + i.
//
// Alignment: the arrays start 256-B aligned, so a group of four positions at i is a 16-B (fp64: 32-B) access for the low members
// iff i % 4 == 0 and for the high ones iff (n + i) % 4 == 0.  Both hold together only when n % 4 == 0: such a level moves in whole
// groups of four (pieces start at multiples of 4); a level with n % 4 != 0 goes value by value, one position per lane -- 4-B
// (8-B) accesses that are still contiguous across the wavefront.

constexpr int kVolGroupThreads = 256;
constexpr int kVolGroupMembers = 8;  // the seven keys in `num` order, then A

// Passed by value in the kernel-argument segment; built once with the layout.  Level l (index l - 1): m[k] = sub-band key k,
// m[7] = A_L at the last level and null below it (an intermediate is no member); n = positions; its pieces of `chunk` positions
// are the workgroups blk[l - 1] .. blk[l] - 1.
struct VolGroupTable {
    int nlevels;
    long long chunk;
    real_t* m[kVolMaxLevels][kVolGroupMembers];
    long long n[kVolMaxLevels];
    int blk[kVolMaxLevels + 1];
};

// the threshold of every level's groups (volume.cpp: level_thresholds)
struct VolGroupBetas {
    real_t b[kVolMaxLevels];
};

// Appends a level to `t` (level 1 first, on a table whose nlevels is 0; then vol_group_finish): band[b] = the start of band
// array b (0 A, 1 H, 2 V, 3 D) of the level -- pdwt_coeff_ptr(plan, b) of a decimated volume, VolumeSwt::band[4 (l - 1) + b] of
// a stationary one --, n = the values of one sub-band (one depth half).
inline void vol_group_add_level(VolGroupTable& t, real_t* const band[4], long long n, bool last) {
    const int l = t.nlevels++;
    for (int k = 0; k < 7; k++) {
        int half, b;
        vol_key_place(k, &half, &b);
        t.m[l][k] = band[b] + (long long)half * n;
    }
    t.m[l][7] = last ? band[0] : nullptr;
    t.n[l] = n;
}
// The workgroup numbering: pieces of `chunk` positions, a multiple of 1024, at least `min_chunk` and about `target` of them over
// all levels.  Returns the number of positions.
inline long long vol_group_finish(VolGroupTable& t, long long target, long long min_chunk) {
    long long total = 0;
    for (int l = 0; l < t.nlevels; l++) total += t.n[l];
    long long chunk = ((total + target - 1) / target + 1023) / 1024 * 1024;
    if (chunk < min_chunk) chunk = min_chunk;
    t.chunk = chunk;
    long long blocks = 0;
    for (int l = 0; l < t.nlevels; l++) {
        t.blk[l] = (int)blocks;
        blocks += (t.n[l] + chunk - 1) / chunk;  // at most target + nlevels in all
    }
    t.blk[t.nlevels] = (int)blocks;
    return total;
}

// workgroup `blk`: its level (index l - 1) and its piece [*a, *e) of positions
PDWT_DEVICE int vol_group_piece(const VolGroupTable& t, int blk, long long* a, long long* e) {
    int l = 0;
    while (l + 1 < t.nlevels && blk >= t.blk[l + 1]) l++;
    const long long lo = (long long)(blk - t.blk[l]) * t.chunk;
    *a = lo;
    *e = lo + t.chunk < t.n[l] ? lo + t.chunk : t.n[l];
    return l;
}

// head / groups / tail of piece [a, e) of a level of n positions: [*g0, *g1) moves in groups of four, every member on an aligned
// address; [a, *g0) and [*g1, e) go value by value
PDWT_DEVICE void vol_group_split(long long n, long long a, long long e, long long* g0, long long* g1) {
    if (n & 3) {  // the two depth halves have different phases: no group
        *g0 = *g1 = e;
        return;
    }
    long long a4 = (a + 3) & ~3LL, e4 = e & ~3LL;
    if (a4 > e) a4 = e;
    if (e4 < a4) e4 = a4;
    *g0 = a4;
    *g1 = e4;
}

// thread `tid` of `nthreads` over its piece: one(i) for a single position, four(i) for the group i .. i + 3
template <typename FS, typename FV>
PDWT_DEVICE void vol_group_sweep(long long n, long long a, long long e, int tid, int nthreads, FS one, FV four) {
    long long g0, g1;
    vol_group_split(n, a, e, &g0, &g1);
    for (long long i = a + tid; i < g0; i += nthreads) one(i);
    for (long long i = g0 + 4LL * tid; i < g1; i += 4LL * nthreads) four(i);
    for (long long i = g1 + tid; i < e; i += nthreads) one(i);
}

// The sum of squares of a group, member by member, and the factor max(1 - beta / ||g||_2, 0) out of it, in real_t.
//   fp32: the plain sum and the plain formula of group_soft_kernel (ops_kernels.hpp).
//   fp64: the same value by a better conditioned route.  1 - beta / ||g|| cancels where a group is just above its threshold, and
//         a member far larger than what is left of it multiplies the half ulp of beta / ||g|| into the result: on the MI355X
//         the plain formula missed 8 * 2^-52 max(|band|, 1) by a sixth (tests/test_gpu_volume_prox.py, 8 x 8 x 8 stationary,
//         where the survivors of level 1 keep only a small part of their length).  So every product and addition of the sum keeps its rounding
//         error (an fma for the product, Knuth's two-sum for the addition), the square root gets its own error back from the
//         exact remainder, and the factor is (||g|| - beta) / ||g||, whose subtraction is then exact to the last bit: the result
//         is good to about two ulps of ITSELF.  The kernel is bound by memory: the extra flops are free.
struct VolSumSq {
    real_t hi, lo;
};
PDWT_DEVICE void vol_sumsq_add(VolSumSq& s, real_t x) {
#ifdef PDWT_DOUBLE
#pragma clang fp contract(off)  // (the error terms are exact only if no product is fused into a neighbouring sum)
    const double p = x * x, e = fma(x, x, -p);
    const double t = s.hi + p, bb = t - s.hi;
    const double err = (s.hi - (t - bb)) + (p - bb);
    s.hi = t;
    s.lo += e + err;
#else
    s.hi += x * x;
#endif
}
PDWT_DEVICE real_t vol_group_res(const VolSumSq& s, real_t beta) {
#ifdef PDWT_DOUBLE
#pragma clang fp contract(off)
    if (s.hi - s.hi == 0.0) {  // (an overflowed or NaN sum takes the plain formula below)
        const double nrm = sqrt(s.hi + s.lo);
        if (nrm == 0.0) return 0.0;
        const double rest = fma(-nrm, nrm, s.hi) + s.lo;  // sum - nrm^2
        const double d = (nrm - beta) + rest / (2.0 * nrm);
        return fmax(d / nrm, 0.0);
    }
#endif
    const real_t nrm = sqrt(s.hi);
    return nrm == real_t(0) ? real_t(0) : fmax(real_t(1) - beta / nrm, real_t(0));
}
// a member's share of a group_norm term: its square in double
PDWT_DEVICE double vol_group_sq(real_t x) { return (double)x * (double)x; }

#if !defined(PDWT_CPU_EMU) && !defined(PDWT_INLINE_HELPERS_ONLY)  // (ops_kernels.hpp; volume.cpp takes the tables only)

// The histogram pass of the rank select over the pieces of `t`: grid = the pieces (t.blk[nranges], or t.blk[nranges - 1] without
// A_L), 1024 threads; k[0]: the wanted K, n: the swept elements.  As select_hist_bands_kernel for one image: a K that needs no pass
// (0, or n and more) reads nothing; partial counts in a 32-KiB LDS histogram with `copies` words per bin, then one integer
// atomic per non-zero bin.
__global__ void __launch_bounds__(kSelectHistThreads) vol_select_hist_kernel(VolRangeTable t, int pass, const long long* __restrict__ k,
                                                                             unsigned long long n, const SelectState* __restrict__ state,
                                                                             unsigned* __restrict__ hist) {
    __shared__ unsigned lh[kSelectLdsWords];
    select_key_t lo_prefix = 0;
    if (pass == 0) {
        if (select_rank_flag(k[0], n)) return;
    } else {
        if (state[0].empty) return;
        lo_prefix = (select_key_t)state[0].lo_prefix;
    }
    long long a, e;
    const int r = vol_piece(t, blockIdx.x, &a, &e);
    const real_t* base = t.base[r];
    const int bits = select_pass_bits(pass), shift = select_pass_shift(pass), bins = 1 << bits;
    const int copies = kSelectLdsWords >> bits, copy = threadIdx.x & (copies - 1);  // as select_hist_kernel
    for (int i = threadIdx.x; i < kSelectLdsWords; i += kSelectHistThreads) lh[i] = 0;
    __syncthreads();
    unsigned unused = kSelectNoDigit;
    auto one = [&](real_t x) {
        const int d = select_classify(select_key(x), shift, bits, lo_prefix, 0, 0, &unused);
        if (d >= 0) atomicAdd(&lh[d * copies + copy], 1u);
    };
    sweep_range(base, a, e, one, [&](const real4_t& v) {
        one(v.x);
        one(v.y);
        one(v.z);
        one(v.w);
    });
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kSelectHistThreads) {
        unsigned s = 0;
        for (int c = 0; c < copies; c++) s += lh[b * copies + c];
        if (s) atomicAdd(&hist[b], s);
    }
}

// x stays, bit for bit, iff the bit pattern of |x| is at least key[0]; else it becomes +0.0 (keep_bands_kernel's arithmetic).  A
// key of 0 keeps everything: the piece returns before it reads; a key with the sign bit set is reached by nothing: the piece
// writes zeros without reading.
__global__ void __launch_bounds__(kVolKeepThreads) vol_keep_kernel(VolRangeTable t, const select_key_t* __restrict__ key) {
    const select_key_t k = key[0], mag = ~(select_key_t)0 >> 1;
    if (k == 0) return;
    long long a, e;
    const int r = vol_piece(t, blockIdx.x, &a, &e);
    real_t* base = t.base[r];
    if (k > mag) {
        sweep_range(base, a, e, [&](real_t& x) { x = real_t(0); }, [&](real4_t& g) { g = real4_t{real_t(0), real_t(0), real_t(0), real_t(0)}; });
        return;
    }
    sweep_range(base, a, e, [&](real_t& x) { x = vol_keep(x, k); },
                [&](real4_t& g) {
                    real4_t v = g;
                    v.x = vol_keep(v.x, k);
                    v.y = vol_keep(v.y, k);
                    v.z = vol_keep(v.z, k);
                    v.w = vol_keep(v.w, k);
                    g = v;
                });
}

// one wavefront per sub-band: out[num][0..1] = the sums of its slices (v.stats[level - 1][band][slice][2], the depth half's
// slices), lane by lane and then by shuffles: a fixed order
__global__ void __launch_bounds__(64) vol_stats_reduce_kernel(VolLevels v, double* __restrict__ out) {
    int level, half, band;
    vol_locate(blockIdx.x, v.nlevels, &level, &half, &band);
    const int hz = v.half[level - 1];
    const double* p = v.stats[level - 1] + 2 * ((long long)band * 2 * hz + (long long)half * hz);
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < hz; i += 64) {
        s1 += p[2 * i];
        s2 += p[2 * i + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = s1;
        out[2 * blockIdx.x + 1] = s2;
    }
}

// one wavefront: out[0..1] = the sums of stats[num][0..1] over the nbands sub-bands, fixed order
__global__ void __launch_bounds__(64) vol_norms_kernel(const double* __restrict__ stats, int nbands, double* __restrict__ out) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nbands; i += 64) {
        s1 += stats[2 * i];
        s2 += stats[2 * i + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    if (threadIdx.x == 0) {
        out[0] = s1;
        out[1] = s2;
    }
}

// table[num] out of stats[num] = {sum |c|, sum c^2} and sigma[0], one thread per sub-band; num 0 (the approximation) gets NaN
__global__ void __launch_bounds__(64) vol_table_kernel(VolLevels v, const double* __restrict__ stats, const double* __restrict__ sigma,
                                                       int method, double visu, real_t* __restrict__ table) {
    const int num = blockIdx.x * blockDim.x + threadIdx.x;
    if (num > 7 * v.nlevels) return;
    double T = __builtin_nan("");
    if (num > 0) T = vol_threshold(method, stats[2 * num + 1], v.n[(num - 1) / 7], sigma[0], visu);
    table[num] = (real_t)T;
}

// one thread per entry [band][slice] of every level plan's table: the threshold of the sub-band the slice belongs to, NaN for the
// slices of an intermediate
__global__ void __launch_bounds__(256) vol_expand_kernel(VolLevels v, const real_t* __restrict__ table) {
    int at;
    const int level = vol_expand_entry(v, blockIdx.x * blockDim.x + threadIdx.x, &at);
    if (!level) return;
    const int hz = v.half[level - 1], band = at / (2 * hz), img = at - band * 2 * hz;
    const int num = vol_num_of(level, v.nlevels, band, img, hz);
    v.table[level - 1][at] = num < 0 ? (real_t)__builtin_nan("") : table[num];
}

// The seven members of a level (and A when `has_a`) at constant indices, so that nothing is indexed at run time and nothing
// lands in scratch.  F(k, pointer) for k = 0 .. 6, then 7.
#define PDWT_VOL_GROUP_EACH(F) \
    F(0, m0) F(1, m1) F(2, m2) F(3, m3) F(4, m4) F(5, m5) F(6, m6)

// member <- member * max(1 - beta_l / ||g||_2, 0) for every group of every level in ONE launch: grid = t.blk[nlevels] pieces.
__global__ void __launch_bounds__(kVolGroupThreads) vol_group_soft_kernel(VolGroupTable t, VolGroupBetas betas, int with_app) {
    long long a, e;
    const int l = vol_group_piece(t, blockIdx.x, &a, &e);
    real_t* const m0 = t.m[l][0];
    real_t* const m1 = t.m[l][1];
    real_t* const m2 = t.m[l][2];
    real_t* const m3 = t.m[l][3];
    real_t* const m4 = t.m[l][4];
    real_t* const m5 = t.m[l][5];
    real_t* const m6 = t.m[l][6];
    real_t* const ma = with_app ? t.m[l][7] : nullptr;
    const real_t beta = betas.b[l];
    vol_group_sweep(
        t.n[l], a, e, threadIdx.x, kVolGroupThreads,
        [&](long long i) {
            VolSumSq ss = {real_t(0), real_t(0)};
#define PDWT_VG_LOAD(k, p)   \
    const real_t x##k = p[i]; \
    vol_sumsq_add(ss, x##k);
            PDWT_VOL_GROUP_EACH(PDWT_VG_LOAD)
#undef PDWT_VG_LOAD
            real_t xa = real_t(0);
            if (ma) {
                xa = ma[i];
                vol_sumsq_add(ss, xa);
            }
            const real_t res = vol_group_res(ss, beta);
#define PDWT_VG_STORE(k, p) p[i] = x##k * res;
            PDWT_VOL_GROUP_EACH(PDWT_VG_STORE)
#undef PDWT_VG_STORE
            if (ma) ma[i] = xa * res;
        },
        [&](long long i) {
            VolSumSq sx = {real_t(0), real_t(0)}, sy = sx, sz = sx, sw = sx;
#define PDWT_VG_LOAD(k, p)                                   \
    real4_t v##k = *reinterpret_cast<const real4_t*>(p + i); \
    vol_sumsq_add(sx, v##k.x), vol_sumsq_add(sy, v##k.y), vol_sumsq_add(sz, v##k.z), vol_sumsq_add(sw, v##k.w);
            PDWT_VOL_GROUP_EACH(PDWT_VG_LOAD)
#undef PDWT_VG_LOAD
            real4_t va = real4_t{real_t(0), real_t(0), real_t(0), real_t(0)};
            if (ma) {
                va = *reinterpret_cast<const real4_t*>(ma + i);
                vol_sumsq_add(sx, va.x), vol_sumsq_add(sy, va.y), vol_sumsq_add(sz, va.z), vol_sumsq_add(sw, va.w);
            }
            const real_t rx = vol_group_res(sx, beta), ry = vol_group_res(sy, beta), rz = vol_group_res(sz, beta), rw = vol_group_res(sw, beta);
#define PDWT_VG_STORE(k, p)                                       \
    v##k.x *= rx, v##k.y *= ry, v##k.z *= rz, v##k.w *= rw;       \
    *reinterpret_cast<real4_t*>(p + i) = v##k;
            PDWT_VOL_GROUP_EACH(PDWT_VG_STORE)
#undef PDWT_VG_STORE
            if (ma) {
                va.x *= rx, va.y *= ry, va.z *= rz, va.w *= rw;
                *reinterpret_cast<real4_t*>(ma + i) = va;
            }
        });
}

// partial[blk] = the sum of ||g||_2 over the workgroup's piece: every term in double (the members' squares converted first, one
// double sqrt), added in a fixed order -- a lane's own terms, wave shuffles, one LDS step.  Reads only.
__global__ void __launch_bounds__(kVolGroupThreads) vol_group_norm_kernel(VolGroupTable t, int with_app, double* __restrict__ partial) {
    long long a, e;
    const int l = vol_group_piece(t, blockIdx.x, &a, &e);
    const real_t* const m0 = t.m[l][0];
    const real_t* const m1 = t.m[l][1];
    const real_t* const m2 = t.m[l][2];
    const real_t* const m3 = t.m[l][3];
    const real_t* const m4 = t.m[l][4];
    const real_t* const m5 = t.m[l][5];
    const real_t* const m6 = t.m[l][6];
    const real_t* const ma = with_app ? t.m[l][7] : nullptr;
    double s = 0.0;
    vol_group_sweep(
        t.n[l], a, e, threadIdx.x, kVolGroupThreads,
        [&](long long i) {
            double ss = 0.0;
#define PDWT_VG_LOAD(k, p) ss += vol_group_sq(p[i]);
            PDWT_VOL_GROUP_EACH(PDWT_VG_LOAD)
#undef PDWT_VG_LOAD
            if (ma) ss += vol_group_sq(ma[i]);
            s += sqrt(ss);
        },
        [&](long long i) {
            double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
#define PDWT_VG_LOAD(k, p)                                                   \
    {                                                                        \
        const real4_t v = *reinterpret_cast<const real4_t*>(p + i);          \
        sx += vol_group_sq(v.x), sy += vol_group_sq(v.y), sz += vol_group_sq(v.z), sw += vol_group_sq(v.w); \
    }
            PDWT_VOL_GROUP_EACH(PDWT_VG_LOAD)
#undef PDWT_VG_LOAD
            if (ma) {
                const real4_t v = *reinterpret_cast<const real4_t*>(ma + i);
                sx += vol_group_sq(v.x), sy += vol_group_sq(v.y), sz += vol_group_sq(v.z), sw += vol_group_sq(v.w);
            }
            s += sqrt(sx);
            s += sqrt(sy);
            s += sqrt(sz);
            s += sqrt(sw);
        });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double part[kVolGroupThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one wavefront: out[0] = the sum of the workgroups' partial sums, in a fixed order
__global__ void __launch_bounds__(64) vol_group_norm_final_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 64) s += partial[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (threadIdx.x == 0) out[0] = s;
}

#undef PDWT_VOL_GROUP_EACH

#endif  // !PDWT_CPU_EMU && !PDWT_INLINE_HELPERS_ONLY

}  // namespace pdwt
