// emu_tail.inc -- the whole-transform-in-one-workgroup kernels: all remaining levels of a small approximation (dwt2_tail_kernels.hpp),
// the whole SWT of a tiny image (swt2_tail_kernels.hpp), all levels of G short rows per wavefront (dwt1_rows_kernels.hpp).
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).
//
// Each runner has an inner function that takes one pointer per plane; the EMU_API entry point packs the planes into det / app as
// before and wraps it.  The emulated LDS is what the launcher asks for, plus EMU_SLACK.

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/dwt1_rows_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_tail_kernels.hpp"
#include "../../pypwt_amd/csrc/swt2_tail_kernels.hpp"

// the unrolled filter lengths that are instantiated (a sanitizer program names fewer: its compile time); every other length runs
// through the run-time-length instantiation
#ifndef EMU_TAIL_HLENS
#define EMU_TAIL_HLENS(X) X(2) X(4) X(6) X(8)
#endif
#ifndef EMU_ROWS_TAIL_HLENS
#define EMU_ROWS_TAIL_HLENS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20)
#endif

// ------------------------------------------------------------------ all remaining levels of a small approximation in one launch
template <int HLEN>
static void run_tail_emu(const TailArgs& a, int batch, bool inverse, int threads, float* smem) {
    for (int bz = 0; bz < batch; bz++) {
        if (inverse) { if (threads == 1024) dwt2_inv_tail_image<HLEN, 1024>(a, bz, smem); else if (threads == 64) dwt2_inv_tail_image<HLEN, 64>(a, bz, smem); else dwt2_inv_tail_image<HLEN, 256>(a, bz, smem); }
        else { if (threads == 1024) dwt2_fwd_tail_image<HLEN, 1024>(a, bz, smem); else if (threads == 64) dwt2_fwd_tail_image<HLEN, 64>(a, bz, smem); else dwt2_fwd_tail_image<HLEN, 256>(a, bz, smem); }
    }
}
template <int HLEN>
static void run_tail_emu_p2(const TailArgs& a, int batch, bool inverse, int threads, float* smem) {
    for (int bz = 0; bz < batch; bz++) {
        if (inverse) { if (threads == 1024) dwt2_inv_tail_image_p2<HLEN, 1024>(a, bz, smem); else if (threads == 64) dwt2_inv_tail_image_p2<HLEN, 64>(a, bz, smem); else dwt2_inv_tail_image_p2<HLEN, 256>(a, bz, smem); }
        else { if (threads == 1024) dwt2_fwd_tail_image_p2<HLEN, 1024>(a, bz, smem); else if (threads == 64) dwt2_fwd_tail_image_p2<HLEN, 64>(a, bz, smem); else dwt2_fwd_tail_image_p2<HLEN, 256>(a, bz, smem); }
    }
}
template <int HLEN>
static void run_tail_emu2(const TailArgs& a, int batch, bool inverse, int threads, size_t lds) {
    const bool p2 = a.lgR >= 0 && a.lgC >= 0;
    // the launcher's dynamic LDS: tail_lds_elems for the mask / shift kernels, tail_geometry for the general ones
    std::vector<float> smem((p2 ? tail_lds_elems(a.R0 * a.C0) : lds) + EMU_SLACK, NAN);
    if (p2) run_tail_emu_p2<HLEN>(a, batch, inverse, threads, smem.data());  // the mask / shift kernels
    else run_tail_emu<HLEN>(a, batch, inverse, threads, smem.data());        // the general ones (unrolled == 2: also for powers of two)
}
// det[3 k + b]: band b (H, V, D) of the group's level k + 1, batch x ceil-halved sizes; app: A_K
static int emu_dwt2_tail_planes(int inverse, float* image, int batch, int R0, int C0, int K, const float* lo, const float* hi, int hlen,
                                int threads, int unrolled, float* const* det, float* app) {
    auto lg2 = [](int v) { int lg = 0; while ((1 << lg) < v) lg++; return (1 << lg) == v ? lg : -1; };
    if ((hlen & 1) || K < 1 || K > kTailMaxLevels) return -2;
    if ((long long)R0 * C0 > kTailTrips * threads || (long long)R0 * C0 > kTailMaxSamples) return -2;
    TailArgs a;
    a.R0 = R0; a.C0 = C0; a.lgR = lg2(R0); a.lgC = lg2(C0); a.K = K; a.hlen = hlen;
    if (unrolled == 2) a.lgR = a.lgC = -1;  // power-of-two sizes through the general kernels too
    const size_t lds = tail_geometry(a, inverse != 0);
    if (lds * sizeof(float) > 160 * 1024) return -2;
    for (int k = 0; k < kTailMaxLevels; k++)
        for (int b = 0; b < 3; b++) a.det[k][b] = k < K ? det[3 * k + b] : nullptr;
    a.in = inverse ? app : image;
    a.out = inverse ? image : app;
    set_bank(a.fb, lo, hi, hlen);
    if (unrolled && hlen <= 8) {
        switch (hlen) {
#define X(h) case h: run_tail_emu2<h>(a, batch, inverse != 0, threads, lds); return 0;
            EMU_TAIL_HLENS(X)
#undef X
        }
    }
    run_tail_emu2<0>(a, batch, inverse != 0, threads, lds);
    return 0;
}
// the sizes of the group's levels, as tail_geometry lays them out: rc[2 k] x rc[2 k + 1] at level k (k = 0: the input)
[[maybe_unused]] static void emu_dwt2_tail_sizes(int R0, int C0, int K, int* rc) {
    TailArgs a;
    a.R0 = R0; a.C0 = C0; a.lgR = a.lgC = -1; a.K = K; a.hlen = 2;
    tail_geometry(a, false);
    for (int k = 0; k <= K; k++) { rc[2 * k] = a.r[k]; rc[2 * k + 1] = a.c[k]; }
}
// det: H,V,D of the group's level 1 (3 x batch x ceil(R0/2) x ceil(C0/2)), then of level 2, ...; app: A_K (sizes by ceil-halving)
EMU_API int emu_dwt2_tail(int inverse, float* image, int batch, int R0, int C0, int K, const float* lo, const float* hi, int hlen,
                          int threads, int unrolled, float* det, float* app) {
    if (K < 1 || K > kTailMaxLevels) return -2;
    int rc[2 * (kTailMaxLevels + 1)];
    emu_dwt2_tail_sizes(R0, C0, K, rc);
    float* d[3 * kTailMaxLevels] = {};
    long long off = 0;
    for (int k = 0; k < K; k++) {
        const long long n = (long long)batch * rc[2 * k + 2] * rc[2 * k + 3];
        for (int b = 0; b < 3; b++) { d[3 * k + b] = det + off; off += n; }
    }
    return emu_dwt2_tail_planes(inverse, image, batch, R0, C0, K, lo, hi, hlen, threads, unrolled, d, app);
}

// ------------------------------------------------------------------ all levels of G short rows per one-wavefront workgroup
template <int HLEN>
static void run_rows_tail_emu(const RowsTailArgs& a, bool inverse, float* smem) {
    const int blocks = (a.rows + a.G - 1) / a.G;
    for (int b = 0; b < blocks; b++) {
        if (inverse) dwt1_rows_tail_inv<HLEN, 64>(a, b, smem);
        else dwt1_rows_tail_fwd<HLEN, 64>(a, b, smem);
    }
}
// det[k]: D_{k+1} (rows x N0 >> (k + 1)); app: A_K
static int emu_dwt1_rows_tail_planes(int inverse, float* data, int rows, int N0, int K, int G, const float* lo, const float* hi, int hlen,
                                     int unrolled, float* const* det, float* app) {
    if ((hlen & 1) || K < 1 || K > kRowsTailMaxLevels || G < 1 || G * N0 > kRowsTailSamples || (N0 % (1 << K))) return -2;
    RowsTailArgs a;
    for (int k = 0; k < kRowsTailMaxLevels; k++) a.det[k] = k < K ? det[k] : nullptr;
    a.in = inverse ? app : data;
    a.out = inverse ? data : app;
    a.rows = rows; a.N0 = N0; a.K = K; a.G = G; a.hlen = hlen;
    set_bank(a.fb, lo, hi, hlen);
    std::vector<float> smem(rows_tail_lds_elems(G * N0) + EMU_SLACK, NAN);
    if (unrolled && hlen <= 20) {
        switch (hlen) {
#define X(h) case h: run_rows_tail_emu<h>(a, inverse != 0, smem.data()); return 0;
            EMU_ROWS_TAIL_HLENS(X)
#undef X
        }
    }
    run_rows_tail_emu<0>(a, inverse != 0, smem.data());
    return 0;
}
// data: forward input / inverse output (rows x N0); det: D_1 (rows x N0/2), D_2, ...; app: A_K
EMU_API int emu_dwt1_rows_tail(int inverse, float* data, int rows, int N0, int K, int G, const float* lo, const float* hi, int hlen,
                               int unrolled, float* det, float* app) {
    if (K < 1 || K > kRowsTailMaxLevels) return -2;
    float* d[kRowsTailMaxLevels] = {};
    long long off = 0;
    for (int k = 0; k < K; k++) { d[k] = det + off; off += (long long)rows * (N0 >> (k + 1)); }
    return emu_dwt1_rows_tail_planes(inverse, data, rows, N0, K, G, lo, hi, hlen, unrolled, d, app);
}

// ------------------------------------------------------------------ the whole SWT of a tiny image in one launch
// det[3 l + b]: band b (H, V, D) of level l + 1 (batch x Nr x Nc); app: A_L
static int emu_swt2_tail_planes(int inverse, float* image, int batch, int Nr, int Nc, int L, const float* lo, const float* hi, int hlen,
                                const float* beta, float* const* det, float* app) {
    if (L < 1 || L > kSwtTailMaxLevels || Nr < 2 || Nc < 2 || (long long)Nr * Nc > kSwtTailMaxSamples) return -2;
    const long long n = (long long)Nr * Nc;
    SwtTailArgs a;
    for (int l = 0; l < kSwtTailMaxLevels; l++) {
        for (int b = 0; b < 3; b++) a.det[l][b] = l < L ? det[3 * l + b] : nullptr;
        a.beta[l] = (beta && l < L) ? beta[l] : 0.f;
    }
    a.in = inverse ? app : image;
    a.out = inverse ? image : app;
    a.R = Nr; a.C = Nc; a.L = L; a.hlen = hlen;
    set_bank(a.fb, lo, hi, hlen);
    std::vector<float> smem(swt_tail_lds_elems((int)n, inverse != 0) + EMU_SLACK, NAN);
    int lgC = 0, lgR = 0;
    while ((1 << lgC) < Nc) lgC++;
    while ((1 << lgR) < Nr) lgR++;
    const bool pow2 = (1 << lgC) == Nc && (1 << lgR) == Nr;
    a.lgC = pow2 ? lgC : -1;
    a.lgR = pow2 ? lgR : -1;
    const bool general = !pow2 || (beta && beta[0] < 0);  // (a negative first threshold: powers of two through the general kernels too)
    if (beta && beta[0] < 0) a.beta[0] = 0.f;
    // the launcher's three shapes: 256 threads x 16 staging trips; 256 x 4 (images of at most 1024 samples); one wavefront x 4 (at most 256)
    const int shape = n <= kSwtTailWaveSamples ? (batch & 1 ? 2 : 1) : (n <= 1024 ? (batch & 1) : 0);
    for (int bz = 0; bz < batch; bz++) {
        if (shape == 2) {
            if (inverse) { if (!general) swt2_inv_tail_image_p2<64, 4>(a, bz, smem.data()); else swt2_inv_tail_image<64, false, 4>(a, bz, smem.data()); }
            else { if (!general) swt2_fwd_tail_image_p2<64, 4>(a, bz, smem.data()); else swt2_fwd_tail_image<64, false, 4>(a, bz, smem.data()); }
        } else if (shape == 1) {
            if (inverse) { if (!general) swt2_inv_tail_image_p2<256, 4>(a, bz, smem.data()); else swt2_inv_tail_image<256, false, 4>(a, bz, smem.data()); }
            else { if (!general) swt2_fwd_tail_image_p2<256, 4>(a, bz, smem.data()); else swt2_fwd_tail_image<256, false, 4>(a, bz, smem.data()); }
        } else {
            if (inverse) { if (!general) swt2_inv_tail_image_p2<256>(a, bz, smem.data()); else swt2_inv_tail_image<256, false>(a, bz, smem.data()); }
            else { if (!general) swt2_fwd_tail_image_p2<256>(a, bz, smem.data()); else swt2_fwd_tail_image<256, false>(a, bz, smem.data()); }
        }
    }
    return 0;
}
// det: H,V,D of level 1 (3 x batch x n), then of level 2, ...; app: A_L (batch x n)
EMU_API int emu_swt2_tail(int inverse, float* image, int batch, int Nr, int Nc, int L, const float* lo, const float* hi, int hlen,
                          const float* beta, float* det, float* app) {
    if (L < 1 || L > kSwtTailMaxLevels) return -2;
    float* d[3 * kSwtTailMaxLevels] = {};
    for (int l = 0; l < L; l++)
        for (int b = 0; b < 3; b++) d[3 * l + b] = det + (3LL * l + b) * batch * Nr * Nc;
    return emu_swt2_tail_planes(inverse, image, batch, Nr, Nc, L, lo, hi, hlen, beta, d, app);
}
