// select_kernels.hpp -- exact order statistics of |c| on the device: a radix select on the bit pattern (gfx950).
//
// The noise level of a wavelet denoiser is sigma = median(|D1|) / 0.6745 (Donoho and Johnstone).  For non-negative IEEE
// values the bit pattern orders like the value (NaNs behind +inf), so the element of a given rank is found digit by digit
// from the top: three passes for fp32 (31 significant bits: 11 + 10 + 10), six for fp64 (63: 11 + 11 + 11 + 10 + 10 + 10).
// A pass is
//   select_hist_kernel   a histogram of this pass's digit over the elements whose higher digits equal the prefix found so
//                        far: per-workgroup LDS histograms, integer adds only, so the result does not depend on the order
//                        in which workgroups arrive;
//   select_walk_kernel   one workgroup per image: walks the bins to the bucket that holds the wanted rank and leaves prefix
//                        and remaining rank in device memory for the next pass.
// No host round trip between passes.
//
// The same passes select ANY rank (best K-term approximation: the K-th largest |c| over several bands of an image):
//   select_hist_bands_kernel  the histogram sweep over the pieces of a BandTable, every piece into the histogram of ITS image;
//   select_walk_rank_kernel   the walk for the ascending rank N - K[image] instead of the median ranks; it also adds up how
//                             many elements lie BELOW the bucket it descends into, so that after the last pass N minus that
//                             sum is the number of elements with key >= the selected one -- ties included, no second sweep.
//
// The median of an even count needs the ranks r and r + 1, which may part in any pass.  Only r is selected.  While r + 1
// lies in the same bucket it shares the prefix (hi_mode 0); when it does not, it is the SMALLEST element of the next
// non-empty bucket, and from then on the histogram sweep also keeps the minimum digit under that second prefix (hi_mode 1):
// one compare per element, no second histogram and no extra sweep.
//
// The digit, bucket-walk and rank logic are plain inline functions that also compile with g++ -DPDWT_CPU_EMU
// (tests/cpu_emu/emu_select.cpp drives them on the host against np.sort); the two kernels are thin wrappers around them.
#pragma once

#include <stdint.h>

#include "kernels_common.hpp"
#ifndef PDWT_CPU_EMU
#include "ops_kernels.hpp"  // sweep_range
#endif

namespace pdwt {

#ifdef PDWT_DOUBLE
typedef unsigned long long select_key_t;
constexpr int kSelectPasses = 6;
constexpr int kSelectKeyBits = 63;
#else
typedef unsigned int select_key_t;
constexpr int kSelectPasses = 3;
constexpr int kSelectKeyBits = 31;
#endif
constexpr int kSelectMaxBins = 2048;   // 11-bit digits at most
constexpr int kSelectLdsWords = 8192;  // LDS histogram of a workgroup: 8192 / bins copies of every bin
constexpr unsigned kSelectNoDigit = 0xffffffffu;
constexpr int kSelectHistThreads = 1024;  // a histogram workgroup: sixteen wavefronts share (zero, fill, flush) one LDS histogram

// per image, in device memory between the passes
struct SelectState {
    unsigned long long lo_prefix;  // the digits of the lower middle element found so far
    unsigned long long hi_prefix;  // hi_mode 1: those of the upper middle element
    unsigned long long lo_rank;    // rank of the lower middle element among the elements under lo_prefix
    unsigned long long count;      // elements that take part (all, or all but the zeros)
    unsigned zeros;                // pass 0: elements whose key is 0 (+0.0 and -0.0), added up by the histogram sweep
    unsigned hi_min;               // hi_mode 1: smallest digit of this pass under hi_prefix, min'ed by the histogram sweep
    int hi_mode;                   // 0: the upper element shares lo's bucket; 1: it is the minimum under hi_prefix; 2: it IS lo
    int empty;                     // no element takes part: the result is 0
    unsigned long long below;      // rank select: elements whose key is smaller than every key under lo_prefix, over the passes
};

PDWT_DEVICE int select_pass_bits(int pass) {
#ifdef PDWT_DOUBLE
    return pass < 3 ? 11 : 10;
#else
    return pass < 1 ? 11 : 10;
#endif
}
// number of key bits below this pass's digit
PDWT_DEVICE int select_pass_shift(int pass) {
    int s = kSelectKeyBits;
    for (int p = 0; p <= pass; p++) s -= select_pass_bits(p);
    return s;
}

// bit pattern of |x|: orders like |x| for every non-NaN value, NaNs behind +inf, -0.0 == +0.0 == 0
PDWT_DEVICE select_key_t select_key(real_t x) {
    select_key_t u;
    __builtin_memcpy(&u, &x, sizeof(u));
    return u & (~(select_key_t)0 >> 1);
}
PDWT_DEVICE real_t select_value(select_key_t key) {
    real_t x;
    __builtin_memcpy(&x, &key, sizeof(x));
    return x;
}

// What one element adds in `pass`: its digit when its higher digits equal lo_prefix (else -1); in hi_mode 1 its digit also
// lowers *hi_min when its higher digits equal hi_prefix.
PDWT_DEVICE int select_classify(select_key_t key, int shift, int bits, select_key_t lo_prefix, int hi_mode, select_key_t hi_prefix,
                                unsigned* hi_min) {
    const select_key_t top = key >> (shift + bits);
    const unsigned digit = (unsigned)(key >> shift) & ((1u << bits) - 1u);
    if (hi_mode == 1 && top == hi_prefix && digit < *hi_min) *hi_min = digit;
    return top == lo_prefix ? (int)digit : -1;
}

// The walk is hierarchical so that one thread finds a bucket among 2048 in about forty reads: part[t] = sum of the bins
// [t per, (t + 1) per), per = bins / 256; part16[g] = sum of part[16 g .. 16 g + 16).
PDWT_DEVICE unsigned select_part_sum(const unsigned* h, int bins, int t) {
    const int per = bins >> 8;
    unsigned s = 0;
    for (int j = 0; j < per; j++) s += h[t * per + j];
    return s;
}
PDWT_DEVICE unsigned select_part16_sum(const unsigned* part, int g) {
    unsigned s = 0;
    for (int j = 0; j < 16; j++) s += part[16 * g + j];
    return s;
}

// the bin whose cumulative count first exceeds `rank`; *below = the count of all bins before it
PDWT_DEVICE int select_descend(const unsigned* h, const unsigned* part, const unsigned* part16, int bins, unsigned long long rank,
                               unsigned long long* below) {
    const int per = bins >> 8;
    unsigned long long cum = 0;
    int g = 0;
    for (; g < 15; g++) {
        if (cum + part16[g] > rank) break;
        cum += part16[g];
    }
    int t = 16 * g;
    for (const int e = t + 15; t < e; t++) {
        if (cum + part[t] > rank) break;
        cum += part[t];
    }
    int b = t * per;
    for (const int e = b + per - 1; b < e; b++) {
        if (cum + h[b] > rank) break;
        cum += h[b];
    }
    *below = cum;
    return b;
}

PDWT_DEVICE int select_first_in_part(const unsigned* h, int per, int t) {
    for (int b = t * per; b < (t + 1) * per; b++)
        if (h[b]) return b;
    return -1;
}
// the first non-empty bin above `bin`, -1 when there is none
PDWT_DEVICE int select_next_nonempty(const unsigned* h, const unsigned* part, const unsigned* part16, int bins, int bin) {
    const int per = bins >> 8, t = bin / per, g = t >> 4;
    for (int b = bin + 1; b < (t + 1) * per; b++)
        if (h[b]) return b;
    for (int tt = t + 1; tt < 16 * (g + 1); tt++)
        if (part[tt]) return select_first_in_part(h, per, tt);
    for (int gg = g + 1; gg < 16; gg++)
        if (part16[gg])
            for (int tt = 16 * gg; tt < 16 * (gg + 1); tt++)
                if (part[tt]) return select_first_in_part(h, per, tt);
    return -1;
}

// The ranks of the median of `count` elements that sit behind `offset` smaller ones: the lower middle element, and whether
// there is an upper one.  (Another quantile is another line here: the walk takes any rank.)
PDWT_DEVICE void select_median_ranks(SelectState& st, unsigned long long offset, unsigned long long count) {
    st.count = count;
    st.empty = count == 0;
    st.lo_rank = offset + (count ? (count - 1) / 2 : 0);
    st.hi_mode = (count & 1) ? 2 : 0;
}

// One pass's walk: h holds the counts of this pass's digit among the elements under st.lo_prefix (part, part16: its partial
// sums), st.zeros and st.hi_min what the sweep left.  n = elements swept per image.
PDWT_DEVICE void select_step(SelectState& st, int pass, const unsigned* h, const unsigned* part, const unsigned* part16, long long n,
                             int skip_zeros) {
    const int bits = select_pass_bits(pass), bins = 1 << bits;
    if (pass == 0) {
        // exact zeros are the smallest keys: leaving them out of the count moves the ranks up by their number
        const unsigned long long zeros = skip_zeros ? st.zeros : 0;
        st.lo_prefix = st.hi_prefix = 0;
        select_median_ranks(st, zeros, (unsigned long long)n - zeros);
    }
    if (st.empty) return;
    unsigned long long below = 0;
    const int bin = select_descend(h, part, part16, bins, st.lo_rank, &below);
    const unsigned long long r = st.lo_rank - below;
    if (st.hi_mode == 0) {
        if (r + 1 >= h[bin]) {  // the upper middle element is the smallest one of the next non-empty bucket
            const int nb = select_next_nonempty(h, part, part16, bins, bin);
            if (nb < 0) st.hi_mode = 2;  // (cannot happen: rank r + 1 exists)
            else {
                st.hi_mode = 1;
                st.hi_prefix = (st.lo_prefix << bits) | (unsigned)nb;
            }
        }
    } else if (st.hi_mode == 1) {
        st.hi_prefix = (st.hi_prefix << bits) | (st.hi_min & ((1u << bits) - 1u));
    }
    st.hi_min = kSelectNoDigit;
    st.lo_prefix = (st.lo_prefix << bits) | (unsigned)bin;
    st.lo_rank = r;
}

// after the last pass: the middle element, or the mean (in double) of the two middle elements
PDWT_DEVICE double select_median(const SelectState& st) {
    if (st.empty) return 0.0;
    const select_key_t lo = (select_key_t)st.lo_prefix, hi = st.hi_mode == 1 ? (select_key_t)st.hi_prefix : lo;
    const double a = (double)select_value(lo);
    if (hi == lo) return a;
    return (a + (double)select_value(hi)) * 0.5;
}

// ---- a given rank: the K-th largest of n elements (K from the caller, any value >= 0)
constexpr int kSelectKeepAll = 1;   // K >= n: every element is "at least as large", the threshold is 0
constexpr int kSelectKeepNone = 2;  // K == 0: no element is, the threshold is +inf
// a key that no element reaches (the sign bit is never set in a key): what the keep sweep compares against when K == 0
constexpr select_key_t kSelectKeyNone = ~(select_key_t)0;

// K clamped to [0, n]; the two ends need no pass at all
PDWT_DEVICE int select_rank_flag(long long k, unsigned long long n) {
    if (k <= 0) return kSelectKeepNone;
    return (unsigned long long)k >= n ? kSelectKeepAll : 0;
}

// One pass's walk for the K-th largest of n elements, i.e. ascending rank n - K: as select_step, without the second middle
// element and without the zeros, and with the count of what lies below the chosen bucket added up in st.below.
PDWT_DEVICE void select_rank_step(SelectState& st, int pass, const unsigned* h, const unsigned* part, const unsigned* part16, long long k,
                                  unsigned long long n) {
    const int bits = select_pass_bits(pass), bins = 1 << bits;
    if (pass == 0) {
        st.lo_prefix = st.hi_prefix = 0;
        st.count = n;
        st.empty = select_rank_flag(k, n) != 0;
        st.lo_rank = st.empty ? 0 : n - (unsigned long long)k;
        st.hi_mode = 2;
        st.below = 0;
    }
    if (st.empty) return;
    unsigned long long below = 0;
    const int bin = select_descend(h, part, part16, bins, st.lo_rank, &below);
    st.lo_prefix = (st.lo_prefix << bits) | (unsigned)bin;
    st.lo_rank -= below;
    st.below += below;
}

// after the last pass: the key of the K-th largest element and the number of elements whose key is at least that
PDWT_DEVICE select_key_t select_rank_result(const SelectState& st, long long k, unsigned long long n, unsigned long long* kept) {
    const int flag = select_rank_flag(k, n);
    if (flag == kSelectKeepNone) {
        *kept = 0;
        return kSelectKeyNone;
    }
    if (flag == kSelectKeepAll) {
        *kept = n;
        return 0;
    }
    *kept = n - st.below;
    return (select_key_t)st.lo_prefix;
}
// the threshold a caller sees: the element itself, +inf when nothing is kept
PDWT_DEVICE real_t select_rank_value(select_key_t key) {
    return key == kSelectKeyNone ? (real_t)__builtin_inf() : select_value(key);
}

constexpr double kSigmaDenominator = 0.6744897501960817;  // the 75 % quantile of the standard normal distribution

#if !defined(PDWT_CPU_EMU) && !defined(PDWT_INLINE_HELPERS_ONLY)  // (ops_kernels.hpp)

// grid (slices, batch): workgroup (s, i) sweeps [s chunk, min(n, (s + 1) chunk)) of image i of the band (n values per image); the
// images start `first` values behind `band`, which is 16-B (fp64: 32-B) aligned whatever `first` is (sweep_range)
__global__ void __launch_bounds__(kSelectHistThreads) select_hist_kernel(const real_t* __restrict__ band, long long first, long long n, long long chunk,
                                                          int pass, SelectState* __restrict__ state, unsigned* __restrict__ hist) {
    __shared__ unsigned lh[kSelectLdsWords];
    __shared__ unsigned sh_min, sh_zero;
    const int img = blockIdx.y;
    SelectState* st = state + img;
    select_key_t lo_prefix = 0, hi_prefix = 0;
    int hi_mode = 0;
    if (pass > 0) {
        if (st->empty) return;
        lo_prefix = (select_key_t)st->lo_prefix;
        hi_prefix = (select_key_t)st->hi_prefix;
        hi_mode = st->hi_mode;
    }
    const int bits = select_pass_bits(pass), shift = select_pass_shift(pass), bins = 1 << bits;
    // Noise-like data puts nearly every element of a wavefront into a handful of first-pass bins (the digit is the exponent
    // and three mantissa bits): every bin has 4 (2048 bins) or 8 (1024 bins) copies, chosen by the lane, so that lanes with
    // the same digit mostly add to different LDS words.
    const int copies = kSelectLdsWords >> bits, copy = threadIdx.x & (copies - 1);
    for (int i = threadIdx.x; i < kSelectLdsWords; i += kSelectHistThreads) lh[i] = 0;
    if (threadIdx.x == 0) {
        sh_min = kSelectNoDigit;
        sh_zero = 0;
    }
    __syncthreads();
    const long long a = first + (long long)img * n + (long long)blockIdx.x * chunk;
    long long e = a + chunk;
    if (e > first + (long long)(img + 1) * n) e = first + (long long)(img + 1) * n;
    unsigned my_min = kSelectNoDigit, my_zero = 0;
    auto one = [&](real_t x) {
        const select_key_t key = select_key(x);
        if (pass == 0 && key == 0) my_zero++;
        const int d = select_classify(key, shift, bits, lo_prefix, hi_mode, hi_prefix, &my_min);
        if (d >= 0) atomicAdd(&lh[d * copies + copy], 1u);
    };
    sweep_range(band, a, e, one, [&](const real4_t& v) {
        one(v.x);
        one(v.y);
        one(v.z);
        one(v.w);
    });
    if (my_zero) atomicAdd(&sh_zero, my_zero);
    if (my_min != kSelectNoDigit) atomicMin(&sh_min, my_min);
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kSelectHistThreads) {
        unsigned s = 0;
        for (int c = 0; c < copies; c++) s += lh[b * copies + c];
        if (s) atomicAdd(&hist[(long long)img * kSelectMaxBins + b], s);
    }
    if (threadIdx.x == 0) {
        if (sh_zero) atomicAdd(&st->zeros, sh_zero);
        if (sh_min != kSelectNoDigit) atomicMin(&st->hi_min, sh_min);
    }
}

// one workgroup per image; clears the image's histogram for the next pass; the last pass writes sigma[image] and clears the
// image's state for the next call (state and histograms are zeroed once, when the workspace is allocated)
__global__ void __launch_bounds__(256) select_walk_kernel(int pass, long long n, int skip_zeros, SelectState* __restrict__ state,
                                                          unsigned* __restrict__ hist, double* __restrict__ sigma) {
    __shared__ unsigned h[kSelectMaxBins], part[256], part16[16];
    const int img = blockIdx.x, bins = 1 << select_pass_bits(pass);
    unsigned* gh = hist + (long long)img * kSelectMaxBins;
    for (int b = threadIdx.x; b < bins; b += 256) {
        h[b] = gh[b];
        gh[b] = 0;
    }
    __syncthreads();
    part[threadIdx.x] = select_part_sum(h, bins, threadIdx.x);
    __syncthreads();
    if (threadIdx.x < 16) part16[threadIdx.x] = select_part16_sum(part, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        SelectState st = state[img];
        select_step(st, pass, h, part, part16, n, skip_zeros);
        if (pass == kSelectPasses - 1) {
            sigma[img] = select_median(st) / kSigmaDenominator;
            st = SelectState{};
        }
        state[img] = st;
    }
}

// The histogram sweep over SEVERAL bands: grid = the pieces of `t` (band_piece), 1024 threads; the pieces of the bands before
// `first_band` return before they read, every other piece adds to the histogram of its image.  k[image]: the wanted K;
// n: elements swept per image.  An image whose K needs no pass (0, or n and more) is not read at all.
__global__ void __launch_bounds__(kSelectHistThreads) select_hist_bands_kernel(const real_t* __restrict__ arena, BandTable t, int first_band,
                                                                               int pass, const long long* __restrict__ k, unsigned long long n,
                                                                               const SelectState* __restrict__ state,
                                                                               unsigned* __restrict__ hist) {
    __shared__ unsigned lh[kSelectLdsWords];
    int band, img;
    long long a, e;
    band_piece(t, blockIdx.x, &band, &img, &a, &e);
    if (band < first_band) return;
    select_key_t lo_prefix = 0;
    if (pass == 0) {
        if (select_rank_flag(k[img], n)) return;
    } else {
        if (state[img].empty) return;
        lo_prefix = (select_key_t)state[img].lo_prefix;
    }
    const int bits = select_pass_bits(pass), shift = select_pass_shift(pass), bins = 1 << bits;
    const int copies = kSelectLdsWords >> bits, copy = threadIdx.x & (copies - 1);  // as select_hist_kernel
    for (int i = threadIdx.x; i < kSelectLdsWords; i += kSelectHistThreads) lh[i] = 0;
    __syncthreads();
    unsigned unused = kSelectNoDigit;
    auto one = [&](real_t x) {
        const int d = select_classify(select_key(x), shift, bits, lo_prefix, 0, 0, &unused);
        if (d >= 0) atomicAdd(&lh[d * copies + copy], 1u);
    };
    sweep_range(arena, a, e, one, [&](const real4_t& v) {
        one(v.x);
        one(v.y);
        one(v.z);
        one(v.w);
    });
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kSelectHistThreads) {
        unsigned s = 0;
        for (int c = 0; c < copies; c++) s += lh[b * copies + c];
        if (s) atomicAdd(&hist[(long long)img * kSelectMaxBins + b], s);
    }
}

// one workgroup per image, as select_walk_kernel; the last pass writes key[image] (what the keep sweep compares against),
// threshold[image], kept[image] and clears the image's state
__global__ void __launch_bounds__(256) select_walk_rank_kernel(int pass, const long long* __restrict__ k, unsigned long long n,
                                                               SelectState* __restrict__ state, unsigned* __restrict__ hist,
                                                               select_key_t* __restrict__ key, real_t* __restrict__ threshold,
                                                               unsigned long long* __restrict__ kept) {
    __shared__ unsigned h[kSelectMaxBins], part[256], part16[16];
    const int img = blockIdx.x, bins = 1 << select_pass_bits(pass);
    unsigned* gh = hist + (long long)img * kSelectMaxBins;
    for (int b = threadIdx.x; b < bins; b += 256) {
        h[b] = gh[b];
        gh[b] = 0;
    }
    __syncthreads();
    part[threadIdx.x] = select_part_sum(h, bins, threadIdx.x);
    __syncthreads();
    if (threadIdx.x < 16) part16[threadIdx.x] = select_part16_sum(part, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        SelectState st = state[img];
        select_rank_step(st, pass, h, part, part16, k[img], n);
        if (pass == kSelectPasses - 1) {
            unsigned long long cnt;
            const select_key_t res = select_rank_result(st, k[img], n, &cnt);
            key[img] = res;
            threshold[img] = select_rank_value(res);
            kept[img] = cnt;
            st = SelectState{};
        }
        state[img] = st;
    }
}

#endif  // !PDWT_CPU_EMU && !PDWT_INLINE_HELPERS_ONLY

}  // namespace pdwt
