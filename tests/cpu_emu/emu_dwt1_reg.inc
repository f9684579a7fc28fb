// emu_dwt1_reg.inc -- the 1D DWT of long rows, up to three levels in registers (dwt1_reg_kernels.hpp).
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).
//
// The inner functions take one pointer per detail level; the EMU_API entry points pack them into det as before and wrap them.  The
// inverse's emulated LDS is kReg1LdsFloats plus EMU_SLACK; the forward stages nothing.

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/dwt1_reg_kernels.hpp"

// the filter lengths that are instantiated (a sanitizer program names fewer: its compile time)
#ifndef EMU_REG1_HLENS
#define EMU_REG1_HLENS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20)
#endif

template <int HLEN, int K>
static void run_fwd1d_reg(const Fwd1DRegArgs& a) {
    const long long waves = (long long)a.rows * a.wpr;
    for (long long w = 0; w < waves; w++) dwt1_fwd_reg<HLEN, K>(a, w);
}

// det[k]: D_{k+1} (rows x N0 >> (k + 1)); app: A_K
static int emu_dwt1_fwd_reg_planes(const float* in, int rows, int N0, int K, const float* lo, const float* hi, int hlen,
                                   int bpw, float* const* det, float* app) {
    if ((hlen & 1) || hlen > kReg1MaxHlen || K < 1 || K > kReg1MaxLevels || (N0 % 16) || N0 < 2048) return -2;
    Fwd1DRegArgs a;
    a.in = in; a.app = app; a.rows = rows; a.N0 = N0;
    for (int k = 0; k < kReg1MaxLevels; k++) a.det[k] = k < K ? det[k] : nullptr;
    reg1_fwd_blocks(hlen, K, N0, &a.nblk, &a.nplain);
    a.bpw = bpw;
    a.wpr = (a.nblk + bpw - 1) / bpw;
    set_bank_i(a.fb, lo, hi, hlen);
#define Y(h, k) if (hlen == h && K == k) { run_fwd1d_reg<h, k>(a); return 0; }
#define X(h) Y(h, 1) Y(h, 2) Y(h, 3)
    EMU_REG1_HLENS(X)
#undef X
#undef Y
    return -1;
}

EMU_API int emu_dwt1_fwd_reg(const float* in, int rows, int N0, int K, const float* lo, const float* hi, int hlen,
                             int bpw, float* det, float* app) {
    if (K < 1 || K > kReg1MaxLevels) return -2;
    float* d[kReg1MaxLevels] = {};
    size_t off = 0;
    for (int k = 1; k <= K; k++) { d[k - 1] = det + off; off += (size_t)rows * (N0 >> k); }
    return emu_dwt1_fwd_reg_planes(in, rows, N0, K, lo, hi, hlen, bpw, d, app);
}

template <int HLEN, int K>
static void run_inv1d_reg(const Inv1DRegArgs& a) {
    const long long waves = (long long)a.rows * a.wpr;
    std::vector<float> lds(kReg1LdsFloats + EMU_SLACK, NAN);
    for (long long w = 0; w < waves; w++) dwt1_inv_reg<HLEN, K>(a, w, lds.data());
}

static int emu_dwt1_inv_reg_planes(const float* app, const float* const* det, int rows, int N0, int K, const float* lo, const float* hi,
                                   int hlen, int bpw, float* out) {
    if ((hlen & 1) || hlen > kReg1MaxHlen || K < 1 || K > kReg1MaxLevels || (N0 % 16) || N0 < 2048) return -2;
    Inv1DRegArgs a;
    a.app = app; a.out = out; a.rows = rows; a.N0 = N0;
    for (int k = 0; k < kReg1MaxLevels; k++) a.det[k] = k < K ? det[k] : nullptr;
    reg1_inv_blocks(hlen, K, N0, &a.nblk, &a.nplain);
    a.bpw = bpw;
    a.wpr = (a.nblk + bpw - 1) / bpw;
    set_bank_i(a.fb, lo, hi, hlen);
#define Y(h, k) if (hlen == h && K == k) { run_inv1d_reg<h, k>(a); return 0; }
#define X(h) Y(h, 1) Y(h, 2) Y(h, 3)
    EMU_REG1_HLENS(X)
#undef X
#undef Y
    return -1;
}

EMU_API int emu_dwt1_inv_reg(const float* app, const float* det, int rows, int N0, int K, const float* lo, const float* hi,
                             int hlen, int bpw, float* out) {
    if (K < 1 || K > kReg1MaxLevels) return -2;
    const float* d[kReg1MaxLevels] = {};
    size_t off = 0;
    for (int k = 1; k <= K; k++) { d[k - 1] = det + off; off += (size_t)rows * (N0 >> k); }
    return emu_dwt1_inv_reg_planes(app, d, rows, N0, K, lo, hi, hlen, bpw, out);
}
