// emu_swt_rows.inc -- the a-trous row kernels of swt_split_kernels.hpp as the (batched) 1D transform: separate approximation /
// detail planes; dilations 1, 2 and 4 through the LDS row kernels, 8 and more through the fwd4 / inv4p register kernels.
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).
//
// The emulated LDS is what the launcher asks for (swt_row_lds_floats of the instantiation) plus EMU_SLACK.

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/swt_split_kernels.hpp"

// the filter lengths that are instantiated (a sanitizer program names fewer: its compile time)
#ifndef EMU_SWT_ROWS_HLENS
#define EMU_SWT_ROWS_HLENS(X) X(4) X(6) X(8) X(10) X(12) X(16) X(20) X(26) X(40)
#endif

template <int HLEN, int F>
static void run_swt1_split_lds(const SwtSplitArgs& k, bool inverse, long long nblocks) {
    constexpr int NT = 256;
    std::vector<float> smem((inverse ? swt_row_lds_floats<HLEN, F, 2>(true, NT) : swt_row_lds_floats<HLEN, F>(false, NT)) + EMU_SLACK, NAN);
    for (long long b = 0; b < nblocks; ++b) {
        if (inverse) swt_row_inv_lds_tile<HLEN, F, 2, NT>(k, b, smem.data());
        else swt_row_fwd_lds_tile<HLEN, F, NT>(k, b, smem.data());
    }
}

template <int HLEN>
static void run_swt1_split(const float* in0, const float* in1, int Nr, int Nc, int f, const FilterBank& fb, bool inverse, float* out0, float* out1) {
    constexpr int NT = 256, R = 4;
    SwtSplitArgs k{};
    k.Nr = Nr; k.Nc = Nc; k.f = f; k.batch = 1;
    for (int j = 0; j < HLEN; ++j) k.t.t[j] = mk2(fb.lo[HLEN - 1 - j], fb.hi[HLEN - 1 - j]);
    k.in[0] = in0; k.in[1] = in1; k.out[0] = out0; k.out[1] = out1;
    const long long row_items4 = f >= 4 ? split_row_waves(1, Nr, split_row_items4(Nc, f, R)) : 0;
    const long long row_lds = split_row_lds_waves(1, Nr, Nc);
    auto blocks = [](long long waves) { return (waves + NT / 64 - 1) / (NT / 64); };
    if (f == 1) return run_swt1_split_lds<HLEN, 1>(k, inverse, blocks(row_lds));
    if (f == 2) return run_swt1_split_lds<HLEN, 2>(k, inverse, blocks(row_lds));
    if (f == 4) return run_swt1_split_lds<HLEN, 4>(k, inverse, blocks(row_lds));
    for (long long b = 0; b < blocks(row_items4); ++b) {
        if (inverse) swt_row_inv4p_tile<HLEN, R, NT>(k, b);
        else swt_row_fwd4_tile<HLEN, R, NT>(k, b);
    }
}

EMU_API int emu_swt1_split(int inverse, const float* in0, const float* in1, int Nr, int Nc, int level, const float* lo, const float* hi,
                           int hlen, float* out0, float* out1) {
    const int f = 1 << (level - 1);
    if ((Nc & 3) || Nc < 16 || f >= Nc) return -2;
    FilterBank fb;
    set_bank(fb, lo, hi, hlen);
    switch (hlen) {
#define X(h) case h: run_swt1_split<h>(in0, in1, Nr, Nc, f, fb, inverse != 0, out0, out1); return 0;
        EMU_SWT_ROWS_HLENS(X)
#undef X
    }
    return -1;
}
