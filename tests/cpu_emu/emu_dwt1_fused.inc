// emu_dwt1_fused.inc -- up to four levels of the 1D DWT per tile launch (dwt1_fused_kernels.hpp).
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).
//
// The inner function takes one pointer per detail level; the EMU_API entry point packs them into det as before and wraps it.  The
// emulated LDS is what the launcher asks for, plus EMU_SLACK.

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/dwt1_fused_kernels.hpp"

// the filter lengths that are instantiated (a sanitizer program names fewer: its compile time)
#ifndef EMU_FUSED1D_HLENS
#define EMU_FUSED1D_HLENS(X) EMU_EVEN_HLENS(X)
#endif

template <int HLEN, int TF, int NT>
static void run_fwd1d_fused(Fwd1DFusedArgs a) {
    std::vector<float> smem(fwd1d_fused_lds_floats(TF, HLEN, a.K) + EMU_SLACK, NAN);
    const int tiles = cdiv(a.N0 >> a.K, TF);
    for (int row = 0; row < a.rows; row++)
        for (int bx = 0; bx < tiles; bx++) dwt1_fwd_fused_tile<HLEN, TF, NT>(a, bx, row, smem.data());
}
template <int HLEN, int T0, int NT>
static void run_inv1d_fused(Inv1DFusedArgs a) {
    std::vector<float> smem(inv1d_fused_lds_floats(T0, HLEN, a.K) + EMU_SLACK, NAN);
    const int tiles = cdiv(a.N0, T0);
    for (int row = 0; row < a.rows; row++)
        for (int bx = 0; bx < tiles; bx++) dwt1_inv_fused_tile<HLEN, T0, NT>(a, bx, row, smem.data());
}

// det[k]: D_{k+1} (rows x N0 >> (k + 1)); app: A_K (rows x N0 >> K)
static int emu_dwt1_fused_planes(int inverse, float* io, int rows, int N0, int K, const float* lo, const float* hi, int hlen,
                                 int small, float* const* det, float* app) {
    // (rows of N0 % 2^(K+1) == 0: the forward stores its deepest level in pairs, the inverse stages it in pairs where it must)
    if ((hlen & 1) || (N0 & 3) || K < 0 || (N0 % (1 << (K + 1))) || K > kMaxFusedLevels) return -2;
    // two levels and more, as the launcher sends them: the forward stages its input in 16-B groups from an origin that is 4-aligned
    // only where 4 divides 2^K, the inverse writes whole 8-sample blocks (one level of 8 n + 4 samples would end behind its row)
    if (K < 2) return -2;
    if (!inverse) {
        Fwd1DFusedArgs a;
        a.in = io; a.app = app; a.rows = rows; a.N0 = N0; a.K = K;
        for (int k = 0; k < kMaxFusedLevels; k++) a.det[k] = k < K ? det[k] : nullptr;
        set_bank_i(a.fb, lo, hi, hlen);
        switch (hlen) {
#define X(h) case h: if (small) run_fwd1d_fused<h, 16, 256>(a); else run_fwd1d_fused<h, 128, 256>(a); return 0;
            EMU_FUSED1D_HLENS(X)
#undef X
        }
    } else {
        Inv1DFusedArgs a;
        a.out = io; a.app = app; a.rows = rows; a.N0 = N0; a.K = K;
        for (int k = 0; k < kMaxFusedLevels; k++) a.det[k] = k < K ? det[k] : nullptr;
        set_bank_i(a.fb, lo, hi, hlen);
        switch (hlen) {
#define X(h) case h: if (small) run_inv1d_fused<h, 1024, 256>(a); else run_inv1d_fused<h, 8192, 256>(a); return 0;
            EMU_FUSED1D_HLENS(X)
#undef X
        }
    }
    return -1;
}

// outputs: det = K row-major planes concatenated in level order (each rows x (N0>>k)), app = rows x (N0>>K)
EMU_API int emu_dwt1_fused(int inverse, float* io, int rows, int N0, int K, const float* lo, const float* hi, int hlen,
                           int small, float* det, float* app) {
    if (K < 0 || K > kMaxFusedLevels) return -2;
    float* dptr[kMaxFusedLevels] = {};
    size_t off = 0;
    for (int k = 1; k <= K; k++) { dptr[k - 1] = det + off; off += (size_t)rows * (N0 >> k); }
    return emu_dwt1_fused_planes(inverse, io, rows, N0, K, lo, hi, hlen, small, dptr, app);
}
