// ops_kernels.hpp -- streaming coefficient operators (HBM-bound, 16 B per lane).
//
// All bands of a plan live in one arena with 256-B aligned, zero-padded bands, so
// an operator that treats every band alike sweeps ONE contiguous range with
// real4_t loads/stores (the reference launches one 16x16-thread kernel per level
// or one cuBLAS-v1 call per band, pdwt/src/common.cu:219-371, wt.cu:368-416).
// Padding is zero and every operator here maps 0 -> 0 (soft and linf with beta < 0 do not: the host zeroes the padding again
// after such a sweep, plan.cpp: rezero_padding).
//
// Semantics (restated in oracle/pdwt_oracle.c):
//   soft   x <- copysign(max(|x|-b,0), x)      pdwt/src/common.cu:13-52
//   hard   x <- x * [|x| > b]                  pdwt/src/common.cu:57-97
//   linf   x <- copysign(min(|x|,b), x)        pdwt/src/common.cu:101-137
//   scale  x <- x * s   (shrink: s = 1/(1+b))  pdwt/src/common.cu:347-371
//   group soft threshold                        pdwt/src/common.cu:145-198
//   axpy   dst += alpha*src                     pdwt/src/common.cu:499-526
//   norms  sum|x|, sum x^2                      pdwt/src/wt.cu:368-416
//   circshift                                   pdwt/src/common.cu:202-211
//
// Per (band, image) operators (no reference counterpart; the recipes are skimage.restoration.denoise_wavelet's):
//   band_stats       sum|x|, sum x^2 of every image of every band
//   threshold_bands  soft / hard with a threshold of its own per (band, image)
//   denoise_table    BayesShrink / VisuShrink thresholds out of those sums and a noise level per image
//   keep_bands       best K-term approximation: keep what is at least as large as a per-image order statistic, zero the rest
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launch.hpp"

namespace pdwt {

// PDWT_INLINE_HELPERS_ONLY: a second translation unit (launch_volume_ops.hip) takes sweep_range and band_piece without defining the
// kernels again
#ifndef PDWT_INLINE_HELPERS_ONLY

template <int OP>
__device__ __forceinline__ real_t ew_apply(real_t x, real_t b) {
    if (OP == EW_SOFT) return copysign(fmax(fabs(x) - b, real_t(0)), x);
    if (OP == EW_HARD) return (fabs(x) - b > real_t(0)) ? x : real_t(0);
    if (OP == EW_LINF) return copysign(fmin(fabs(x), b), x);
    return x * b;
}

// n4 = number of real4_t groups; the host only passes 16-B aligned, padded ranges
template <int OP>
__global__ void __launch_bounds__(256) ew_kernel(real4_t* __restrict__ p, long long n4, real_t b) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        real4_t v = p[i];
        v.x = ew_apply<OP>(v.x, b);
        v.y = ew_apply<OP>(v.y, b);
        v.z = ew_apply<OP>(v.z, b);
        v.w = ew_apply<OP>(v.w, b);
        p[i] = v;
    }
}

// nb detail bands (1 or 3) of one level, optional approximation band
__global__ void __launch_bounds__(256) group_soft_kernel(real_t* __restrict__ d0, real_t* __restrict__ d1,
                                                         real_t* __restrict__ d2, real_t* __restrict__ ap,
                                                         long long n, real_t beta, int nb) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const real_t a = d0[i];
        const real_t b = nb > 1 ? d1[i] : real_t(0);
        const real_t c = nb > 1 ? d2[i] : real_t(0);
        const real_t e = ap ? ap[i] : real_t(0);
        const real_t nrm = sqrt(a * a + b * b + c * c + e * e);
        const real_t res = (nrm == real_t(0)) ? real_t(0) : fmax(real_t(1) - beta / nrm, real_t(0));
        d0[i] = a * res;
        if (nb > 1) {
            d1[i] = b * res;
            d2[i] = c * res;
        }
        if (ap) ap[i] = e * res;
    }
}

__global__ void __launch_bounds__(256) axpy_kernel(real4_t* __restrict__ dst, const real4_t* __restrict__ src,
                                                   long long n4, real_t alpha) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        real4_t d = dst[i];
        const real4_t s = src[i];
        d.x = pdwt_fma(alpha, s.x, d.x);
        d.y = pdwt_fma(alpha, s.y, d.y);
        d.z = pdwt_fma(alpha, s.z, d.z);
        d.w = pdwt_fma(alpha, s.w, d.w);
        dst[i] = d;
    }
}

// sum|x| and sum x^2 in two launches without atomics (fp64 accumulation: one wave-shuffle reduction per wavefront, one LDS
// step per block): every block writes its two partial sums to its own slot, one block adds the slots up.  (Rounds 1-3 had
// every block add to ONE pair of doubles with atomicAdd: 4096 same-address fp64 atomics serialise at the memory side --
// norm1 of 2^24 coefficients took 81 us, a twelfth of the streaming rate, found in round 4 by tools/opsbench.py.)
constexpr int kNormsMaxBlocks = 1024;
__global__ void __launch_bounds__(256) norms_partial_kernel(const real4_t* __restrict__ p, long long n4,
                                                            double* __restrict__ partial) {
    double s1 = 0.0, s2 = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const real4_t v = p[i];
        s1 += (double)fabs(v.x) + (double)fabs(v.y) + (double)fabs(v.z) + (double)fabs(v.w);
        s2 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // 64-wide wavefront
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part[0][wave] = s1;
        part[1][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        partial[2 * blockIdx.x + 1] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    }
}
// The inner loop of iterative shrinkage -- soft_threshold, then norm1 of what is left (pdwt/README.md:6-7; wt.cu:308-315,
// 396-416) -- as ONE sweep: x' = soft(x, beta) for every coefficient (beta = b_lo in the first split4 groups -- the
// approximation band --, b_hi behind; keep_lo: the first part as it is), sum |x'| and sum x'^2 per block.  STORE = false is the
// read-only form for plans whose inverse applies the threshold as it loads the details (2D SWT): the norms of the
// thresholded coefficients without touching them.
template <bool STORE>
__global__ void __launch_bounds__(256) soft_norms_partial_kernel(real4_t* __restrict__ p, long long n4, long long split4, real_t b_lo,
                                                                 real_t b_hi, int keep_lo, double* __restrict__ partial) {
    double s1 = 0.0, s2 = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        real4_t v = p[i];
        const bool lo = i < split4;
        if (!(lo && keep_lo)) {
            const real_t b = lo ? b_lo : b_hi;
            v.x = ew_apply<EW_SOFT>(v.x, b);
            v.y = ew_apply<EW_SOFT>(v.y, b);
            v.z = ew_apply<EW_SOFT>(v.z, b);
            v.w = ew_apply<EW_SOFT>(v.w, b);
            if (STORE) p[i] = v;
        }
        s1 += (double)fabs(v.x) + (double)fabs(v.y) + (double)fabs(v.z) + (double)fabs(v.w);
        s2 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part[0][wave] = s1;
        part[1][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        partial[2 * blockIdx.x + 1] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    }
}
// one block: out[0] = sum of partial[2 b], out[1] = sum of partial[2 b + 1], b < nblocks (fixed order: deterministic)
__global__ void __launch_bounds__(256) norms_final_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ out) {
    double s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        s1 += partial[2 * b];
        s2 += partial[2 * b + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part[0][wave] = s1;
        part[1][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        out[1] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    }
}

#endif  // !PDWT_INLINE_HELPERS_ONLY

// ---------------------------------------------------------------------------------------------------------------------
// Operators that tell bands and images apart.  A (band, image) pair is n contiguous values at off[band] + image * n; n is
// not a multiple of 4 in general (61 x 59 planes, batch 3), so the pairs do not start on 16-B boundaries.  The sweep is cut
// into workgroup-sized pieces of ONE pair each (BandTable, launch.hpp): a piece reads single values up to the first whole
// 16-B group, whole groups, and single values behind the last one -- the padding behind a band is never touched.

// [a, e) of p, in elements from a 16-B aligned base (T = real_t or const real_t)
template <typename T, typename FS, typename FV>
__device__ __forceinline__ void sweep_range(T* __restrict__ p, long long a, long long e, FS one, FV four) {
    typedef typename std::conditional<std::is_const<T>::value, const real4_t, real4_t>::type T4;
    long long a4 = (a + 3) & ~3LL, e4 = e & ~3LL;
    if (a4 > e) a4 = e;
    if (e4 < a4) e4 = a4;
    if ((long long)threadIdx.x < a4 - a) one(p[a + threadIdx.x]);
    if ((long long)threadIdx.x < e - e4) one(p[e4 + threadIdx.x]);
    T4* p4 = reinterpret_cast<T4*>(p);
    for (long long i = a4 / 4 + threadIdx.x; i < e4 / 4; i += blockDim.x) four(p4[i]);
}

// workgroup `blk` of a per-pair sweep: its band, its image and its piece [*a, *e) of the arena
__device__ __forceinline__ void band_piece(const BandTable& t, int blk, int* band, int* img, long long* a, long long* e) {
    int b = 0;
    while (b + 1 < t.nbands && blk >= t.blk[b + 1]) b++;
    const long long n = t.n[b], slices = (n + t.chunk - 1) / t.chunk;
    const long long r = blk - t.blk[b], i = r / slices, s = r - i * slices;
    const long long first = t.off[b] + i * n, lo = first + s * t.chunk;
    *band = b;
    *img = (int)i;
    *a = lo;
    *e = lo + t.chunk < first + n ? lo + t.chunk : first + n;
}

#ifndef PDWT_INLINE_HELPERS_ONLY

// partial[2 blk], [2 blk + 1] = sum |x|, sum x^2 over the workgroup's piece (fp64, fixed order: wave shuffles, one LDS step)
__global__ void __launch_bounds__(256) band_stats_partial_kernel(const real_t* __restrict__ arena, BandTable t, double* __restrict__ partial) {
    int band, img;
    long long a, e;
    band_piece(t, blockIdx.x, &band, &img, &a, &e);
    double s1 = 0.0, s2 = 0.0;
    sweep_range(arena, a, e,
                [&](const real_t& x) {
                    s1 += (double)fabs(x);
                    s2 += (double)x * x;
                },
                [&](const real4_t& v) {
                    s1 += (double)fabs(v.x) + (double)fabs(v.y) + (double)fabs(v.z) + (double)fabs(v.w);
                    s2 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
                });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    __shared__ double part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part[0][wave] = s1;
        part[1][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        partial[2 * blockIdx.x + 1] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    }
}
// one wavefront per (band, image): out[band][image][0..1] = the sums of its pieces, in a fixed order
__global__ void __launch_bounds__(64) band_stats_final_kernel(const double* __restrict__ partial, BandTable t, double* __restrict__ out) {
    const int band = blockIdx.x / t.batch, img = blockIdx.x - band * t.batch;
    const long long slices = (t.n[band] + t.chunk - 1) / t.chunk;
    const double* p = partial + 2 * ((long long)t.blk[band] + (long long)img * slices);
    double s1 = 0.0, s2 = 0.0;
    for (long long k = threadIdx.x; k < slices; k += 64) {
        s1 += p[2 * k];
        s2 += p[2 * k + 1];
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

// x <- op(x, table[band][image]) for every pair in ONE launch; a NaN entry leaves its pair untouched (and unread)
template <int OP>
__global__ void __launch_bounds__(256) threshold_bands_kernel(real_t* __restrict__ arena, BandTable t, const real_t* __restrict__ table) {
    int band, img;
    long long a, e;
    band_piece(t, blockIdx.x, &band, &img, &a, &e);
    const real_t b = table[(long long)band * t.batch + img];
    if (b != b) return;
    sweep_range(arena, a, e, [&](real_t& x) { x = ew_apply<OP>(x, b); },
                [&](real4_t& r) {
                    real4_t v = r;
                    v.x = ew_apply<OP>(v.x, b);
                    v.y = ew_apply<OP>(v.y, b);
                    v.z = ew_apply<OP>(v.z, b);
                    v.w = ew_apply<OP>(v.w, b);
                    r = v;
                });
}

// Best K-term approximation: x stays, bit for bit, iff the bit pattern of |x| is at least key[image]; else it becomes +0.0.
// KEY is the unsigned integer of real_t's width (select_key_t of select_kernels.hpp, whose walk leaves key[image] in device
// memory): NaNs order behind +inf, ties at the key all survive.  Pieces of the bands before `first_band` are left alone.  A
// key of 0 keeps everything: the piece returns before it reads; a key with the sign bit set is reached by nothing: the piece
// writes zeros without reading.
template <typename KEY>
__global__ void __launch_bounds__(256) keep_bands_kernel(real_t* __restrict__ arena, BandTable t, int first_band, const KEY* __restrict__ key) {
    static_assert(sizeof(KEY) == sizeof(real_t), "the key is the bit pattern of a value");
    int band, img;
    long long a, e;
    band_piece(t, blockIdx.x, &band, &img, &a, &e);
    if (band < first_band) return;
    const KEY k = key[img], mag = ~(KEY)0 >> 1;
    if (k == 0) return;
    if (k > mag) {
        sweep_range(arena, a, e, [&](real_t& x) { x = real_t(0); }, [&](real4_t& r) { r = real4_t{real_t(0), real_t(0), real_t(0), real_t(0)}; });
        return;
    }
    auto keep = [&](real_t x) {
        KEY u;
        __builtin_memcpy(&u, &x, sizeof(u));
        return (u & mag) >= k ? x : real_t(0);
    };
    sweep_range(arena, a, e, [&](real_t& x) { x = keep(x); },
                [&](real4_t& r) {
                    real4_t v = r;
                    v.x = keep(v.x);
                    v.y = keep(v.y);
                    v.z = keep(v.z);
                    v.w = keep(v.w);
                    r = v;
                });
}

// table[band][image] out of stats[band][image] = {sum |c|, sum c^2} and sigma[image] (skimage.restoration._denoise:
// _bayes_thresh, _universal_thresh), in double, rounded once to real_t; band 0 (the approximation) gets NaN
//   BayesShrink  var / sqrt(max(sumsq / n - var, eps)),  var = sigma^2, eps = the machine epsilon of real_t
//   VisuShrink   sigma * visu, visu = sqrt(2 ln(Nr Nc)) from the host
__global__ void __launch_bounds__(256) denoise_table_kernel(BandTable t, const double* __restrict__ stats, const double* __restrict__ sigma,
                                                            int method, double visu, real_t* __restrict__ table) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= t.nbands * t.batch) return;
    const int band = idx / t.batch, img = idx - band * t.batch;
    double T;
    if (band == 0) {
        T = __builtin_nan("");
    } else if (method == DENOISE_VISU) {
        T = sigma[img] * visu;
    } else {
        const double var = sigma[img] * sigma[img], eps = sizeof(real_t) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;
        const double d = stats[2 * idx + 1] / (double)t.n[band] - var;
        T = var / sqrt(d > eps ? d : eps);
    }
    table[idx] = (real_t)T;
}

// out[b][y][x] = in[b][(y - sr) mod Nr][(x - sc) mod Nc],  0 <= sr < Nr, 0 <= sc < Nc
__global__ void __launch_bounds__(256) circshift_kernel(const real_t* __restrict__ in, real_t* __restrict__ out,
                                                        int Nr, int Nc, int sr, int sc) {
    const long long plane = (long long)Nr * Nc;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < plane) {
        const int y = (int)(idx / Nc), x = (int)(idx - (long long)y * Nc);
        int r = y - sr, c = x - sc;
        if (r < 0) r += Nr;
        if (c < 0) c += Nc;
        const long long b = (long long)blockIdx.y * plane;
        out[b + idx] = in[b + (long long)r * Nc + c];
    }
}

// deterministic test/bench input, identical to oracle_fill_hash and
// tests/golden/make_golden.py:hash_input
__global__ void __launch_bounds__(256) fill_hash_kernel(real_t* __restrict__ x, long long n, uint32_t seed,
                                                        real_t scale, long long index_offset) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t h = (uint32_t)(i + index_offset) ^ seed;
        h ^= h >> 16;
        h *= 0x7FEB352Du;
        h ^= h >> 15;
        h *= 0x846CA68Bu;
        h ^= h >> 16;
        x[i] = (real_t)((float)(h >> 8) * (1.0f / 16777216.0f)) * scale;  // 24-bit value, exact in fp32
    }
}

// plain 16-B grid-stride copy: the measured ceiling a streaming kernel of the same footprint is compared with
// (pdwt_time_copy; MI355X_MICROARCH.md quotes 6.29 TB/s for this kernel shape on buffers far beyond the Infinity Cache)
__global__ void __launch_bounds__(256) copy_kernel(const real4_t* __restrict__ a, real4_t* __restrict__ b, long long n4) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) b[i] = a[i];
}

#endif  // !PDWT_INLINE_HELPERS_ONLY

}  // namespace pdwt
