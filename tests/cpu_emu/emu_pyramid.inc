// emu_pyramid.inc -- the 2D pyramids: two levels per tile launch (dwt2_pyramid_kernels.hpp), three levels of small images
// (dwt2_pyr3_kernels.hpp).
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).
//
// Each runner has an inner function that takes one pointer per plane; the EMU_API entry point packs the planes (l1 = H1|V1|D1,
// l2 = A2|H2|V2|D2, det) as before and wraps it.  The emulated LDS is the geometry's size plus EMU_SLACK.

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/dwt2_pyramid_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_pyr3_kernels.hpp"

// the filter lengths that are instantiated (a sanitizer program names fewer: its compile time)
#ifndef EMU_PYR_HLENS
#define EMU_PYR_HLENS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16)
#endif

// ------------------------------------------------------------------ two-level pyramid (forward)
template <int HLEN, int TX2, int TY2, int NT>
static void run_fwd_pyr2(FwdPyr2Args a, int batch) {
    std::vector<float> smem(Pyr2Geom<HLEN, TX2, TY2>::LDS_FLOATS + EMU_SLACK, NAN);
    a.tiles_x = cdiv(a.N0c / 4, TX2); a.tiles_y = cdiv(a.N0r / 4, TY2);
    for (int bz = 0; bz < batch; bz++)
        for (int by = 0; by < a.tiles_y; by++)
            for (int bx = 0; bx < a.tiles_x; bx++) dwt2_fwd_pyr2_tile<HLEN, TX2, TY2, NT>(a, bx, by, bz, smem.data());
}

// l1[3]: H1, V1, D1 (batch x N0r/2 x N0c/2 each); l2[4]: A2, H2, V2, D2 (batch x N0r/4 x N0c/4 each)
static int emu_dwt2_fwd_pyr2_planes(const float* in, int batch, int N0r, int N0c, const float* lo, const float* hi, int hlen,
                                    int tile, float* const* l1, float* const* l2) {
    if ((hlen & 1) || hlen > 16 || (N0c & 7) || (N0r & 3)) return -2;
    FwdPyr2Args a;
    a.in = in; a.H1 = l1[0]; a.V1 = l1[1]; a.D1 = l1[2];
    a.A2 = l2[0]; a.H2 = l2[1]; a.V2 = l2[2]; a.D2 = l2[3];
    a.N0r = N0r; a.N0c = N0c;
    a.in_bstride = (long long)N0r * N0c; a.l1_bstride = (long long)(N0r / 2) * (N0c / 2);
    a.l2_bstride = (long long)(N0r / 4) * (N0c / 4);
    set_bank_i(a.fb, lo, hi, hlen);
    switch (hlen) {
#define X(h) case h: if (tile == 0) run_fwd_pyr2<h, 32, 4, 256>(a, batch); else run_fwd_pyr2<h, 32, 8, 256>(a, batch); return 0;
        EMU_PYR_HLENS(X)
#undef X
    }
    return -1;
}

// l1: H,V,D planes of the first level (3 x batch x N0r/2 x N0c/2), l2: A,H,V,D of the second (4 x ...)
EMU_API int emu_dwt2_fwd_pyr2(const float* in, int batch, int N0r, int N0c, const float* lo, const float* hi, int hlen,
                              int tile, float* l1, float* l2) {
    const long long n1 = (long long)batch * (N0r / 2) * (N0c / 2), n2 = (long long)batch * (N0r / 4) * (N0c / 4);
    float* const p1[3] = {l1, l1 + n1, l1 + 2 * n1};
    float* const p2[4] = {l2, l2 + n2, l2 + 2 * n2, l2 + 3 * n2};
    return emu_dwt2_fwd_pyr2_planes(in, batch, N0r, N0c, lo, hi, hlen, tile, p1, p2);
}

// ------------------------------------------------------------------ two-level pyramid (inverse)
template <int HLEN, int TX, int TY, int NT>
static void run_inv_pyr2(InvPyr2Args a, int batch) {
    std::vector<float> smem(InvPyr2Geom<HLEN, TX, TY>::LDS_FLOATS + EMU_SLACK, NAN);
    a.tiles_x = cdiv(a.N0c, 2 * TX); a.tiles_y = cdiv(a.N0r, 2 * TY);
    for (int bz = 0; bz < batch; bz++)
        for (int by = 0; by < a.tiles_y; by++)
            for (int bx = 0; bx < a.tiles_x; bx++) dwt2_inv_pyr2_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
}

static int emu_dwt2_inv_pyr2_planes(const float* const* l1, const float* const* l2, int batch, int N0r, int N0c, const float* lo,
                                    const float* hi, int hlen, int tile, float* out) {
    if ((hlen & 1) || hlen > 16 || (N0c & 7) || (N0r & 3)) return -2;
    InvPyr2Args a;
    a.H1 = l1[0]; a.V1 = l1[1]; a.D1 = l1[2];
    a.A2 = l2[0]; a.H2 = l2[1]; a.V2 = l2[2]; a.D2 = l2[3];
    a.out = out; a.N0r = N0r; a.N0c = N0c;
    a.out_bstride = (long long)N0r * N0c; a.l1_bstride = (long long)(N0r / 2) * (N0c / 2);
    a.l2_bstride = (long long)(N0r / 4) * (N0c / 4);
    set_bank_i(a.fb, lo, hi, hlen);
    switch (hlen) {
#define X(h) case h: if (tile == 0) run_inv_pyr2<h, 64, 8, 256>(a, batch); else run_inv_pyr2<h, 64, 16, 256>(a, batch); return 0;
        EMU_PYR_HLENS(X)
#undef X
    }
    return -1;
}

EMU_API int emu_dwt2_inv_pyr2(const float* l1, const float* l2, int batch, int N0r, int N0c, const float* lo,
                              const float* hi, int hlen, int tile, float* out) {
    const long long n1 = (long long)batch * (N0r / 2) * (N0c / 2), n2 = (long long)batch * (N0r / 4) * (N0c / 4);
    const float* const p1[3] = {l1, l1 + n1, l1 + 2 * n1};
    const float* const p2[4] = {l2, l2 + n2, l2 + 2 * n2, l2 + 3 * n2};
    return emu_dwt2_inv_pyr2_planes(p1, p2, batch, N0r, N0c, lo, hi, hlen, tile, out);
}

// ------------------------------------------------------------------ three-level pyramid (small images)
template <int HLEN, int T>
static void run_pyr3(Pyr3Args a, int batch, bool inverse) {
    constexpr int T0 = 8 * T, NT = 256;
    if (!inverse) {
        std::vector<float> smem(Pyr3FwdGeom<HLEN, T>::LDS + EMU_SLACK, NAN);
        a.tiles_x = cdiv(a.N0c / 8, T); a.tiles_y = cdiv(a.N0r / 8, T);
        for (int bz = 0; bz < batch; bz++)
            for (int by = 0; by < a.tiles_y; by++)
                for (int bx = 0; bx < a.tiles_x; bx++) dwt2_fwd_pyr3_tile<HLEN, T, NT>(a, bx, by, bz, smem.data());
    } else {
        std::vector<float> smem(Pyr3InvGeom<HLEN, T0>::LDS + EMU_SLACK, NAN);
        a.tiles_x = cdiv(a.N0c, T0); a.tiles_y = cdiv(a.N0r, T0);
        for (int bz = 0; bz < batch; bz++)
            for (int by = 0; by < a.tiles_y; by++)
                for (int bx = 0; bx < a.tiles_x; bx++) dwt2_inv_pyr3_tile<HLEN, T0, NT>(a, bx, by, bz, smem.data());
    }
}

// det[3 k + b]: band b (H, V, D) of level k + 1 (batch x N0r >> (k + 1) x N0c >> (k + 1)); app: A3
static int emu_dwt2_pyr3_planes(int inverse, float* image, int batch, int N0r, int N0c, const float* lo, const float* hi, int hlen,
                                int tile, float* const* det, float* app) {
    if ((hlen & 1) || hlen > 16 || (N0c & 7) || (N0r & 7)) return -2;
    Pyr3Args a;
    for (int k = 0; k < 3; k++)
        for (int b = 0; b < 3; b++) a.det[k][b] = det[3 * k + b];
    a.in = inverse ? app : image;
    a.out = inverse ? image : app;
    a.N0r = N0r; a.N0c = N0c;
    set_bank(a.fb, lo, hi, hlen);
    switch (hlen) {
#define X(h) case h: if (tile == 2) run_pyr3<h, 2>(a, batch, inverse != 0); else if (tile == 4) run_pyr3<h, 4>(a, batch, inverse != 0); else run_pyr3<h, 8>(a, batch, inverse != 0); return 0;
        EMU_PYR_HLENS(X)
#undef X
    }
    return -1;
}

// det: H,V,D of level 1 (3 x batch x N0r/2 x N0c/2), then of level 2, then of level 3; app: A3 (batch x N0r/8 x N0c/8)
EMU_API int emu_dwt2_pyr3(int inverse, float* image, int batch, int N0r, int N0c, const float* lo, const float* hi, int hlen,
                          int tile, float* det, float* app) {
    float* d[9];
    long long off = 0;
    for (int k = 0; k < 3; k++) {
        const long long n = (long long)batch * (N0r >> (k + 1)) * (N0c >> (k + 1));
        for (int b = 0; b < 3; b++) { d[3 * k + b] = det + off; off += n; }
    }
    return emu_dwt2_pyr3_planes(inverse, image, batch, N0r, N0c, lo, hi, hlen, tile, d, app);
}
