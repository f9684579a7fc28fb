// emu_swt_split.inc -- one a-trous level as a row launch + a column launch through scratch (swt_split_kernels.hpp), the column
// pass optionally as a strip walk (swt_colstream_kernels.hpp, EMU_SPLIT_COLSTREAM).
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/swt_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_split_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_colstream_kernels.hpp"

// the filter lengths that are instantiated (a sanitizer program names fewer: its compile time)
#ifndef EMU_SPLIT_HLENS
#define EMU_SPLIT_HLENS(X) X(4) X(6) X(8) X(10) X(12) X(16) X(20) X(26) X(40)
#endif

// the column pass streamed down strips (swt_colstream_kernels.hpp) on the arguments of the register column kernels
static int g_colstream_runs = 0;
EMU_API int emu_colstream_runs() { return g_colstream_runs; }  // launches that took the strip kernels so far
template <int HLEN, bool INV>
static bool run_swt_colstream(const SwtSplitArgs& c) {
    if constexpr (HLEN < 10) {
        return false;
    } else {
        constexpr int TXC = 64, TY = 32, NT = 256, M = 8;
        using G = SwtColStreamGeom<HLEN, INV, TXC, TY>;
        SwtColStreamArgs a;
        for (int k = 0; k < 4; ++k) { a.in[k] = c.in[k]; a.out[k] = c.out[k]; }
        a.Nr = c.Nr; a.Nc = c.Nc; a.f = c.f; a.in_bstride = c.in_bstride; a.out_bstride = c.out_bstride;
        a.soft_beta = c.soft_beta; a.t = c.t;
        a.wk = swt_walk(c.Nr, c.Nc, c.f, 4);
        if ((c.Nc & 3) || a.wk.rows_phase < TY) return false;
        a.strips = (c.Nc + TXC - 1) / TXC;
        const char* e = getenv("EMU_COLSTREAM_SEG");  // rows of a chain per segment (default: two segments)
        int seg = e ? atoi(e) : (a.wk.rows_phase + 1) / 2;
        a.seg = (seg + TY - 1) / TY * TY;
        a.segs = (a.wk.rows_phase + a.seg - 1) / a.seg;
        std::vector<float> smem(G::LDS_REALS, NAN);
        ++g_colstream_runs;
        for (int bz = 0; bz < c.batch; ++bz)
            for (int py = 0; py < a.wk.phases; ++py)
                for (int sg = 0; sg < a.segs; ++sg)
                    for (int st = 0; st < a.strips; ++st) swt_colstream_wg<HLEN, INV, TXC, TY, NT, M>(a, st, py, sg, bz, smem.data());
        return true;
    }
}

// ---- one a-trous level as a row pass + a column pass through scratch (swt_split_kernels.hpp); planes as in emu_swt2
template <int HLEN>
static void run_swt_split(const Swt2DArgs& a, int batch, bool inverse, float* tmp) {
    constexpr int NT = 256, R = 4;
    const long long plane = (long long)a.Nr * a.Nc;
    SwtSplitArgs k{};
    k.Nr = a.Nr; k.Nc = a.Nc; k.f = a.f; k.batch = batch; k.soft_beta = a.soft_beta;
    for (int j = 0; j < HLEN; ++j) k.t.t[j] = mk2(a.fb.lo[HLEN - 1 - j], a.fb.hi[HLEN - 1 - j]);
    const int f = a.f;
    const long long col_items = split_col_waves(batch, a.Nr, a.Nc, f, R);
    const long long row_items4 = f >= 4 ? split_row_waves(batch, a.Nr, split_row_items4(a.Nc, f, R)) : 0;
    const long long row_lds = split_row_lds_waves(batch, a.Nr, a.Nc);
    std::vector<float> smem(16384, NAN);  // one workgroup's LDS
    const bool direct = getenv("EMU_SPLIT_DIRECT") != nullptr;  // dilation 4 through the kernel of the dilations >= 8 (quads f apart, no LDS)
    const bool colstream = getenv("EMU_SPLIT_COLSTREAM") != nullptr;  // the column passes through swt_colstream_kernels.hpp
    auto blocks = [](long long waves) { return (waves + NT / 64 - 1) / (NT / 64); };
    if (!inverse) {
        SwtSplitArgs r = k;
        r.in[0] = a.in; r.in_bstride = a.bstride; r.out[0] = tmp; r.out[1] = tmp + plane; r.out_bstride = 2 * plane;
        if (f == 1) for (long long b = 0; b < blocks(row_lds); ++b) swt_row_fwd_lds_tile<HLEN, 1, NT>(r, b, smem.data());
        else if (f == 2) for (long long b = 0; b < blocks(row_lds); ++b) swt_row_fwd_lds_tile<HLEN, 2, NT>(r, b, smem.data());
        else if (f == 4 && !direct) for (long long b = 0; b < blocks(row_lds); ++b) swt_row_fwd_lds_tile<HLEN, 4, NT>(r, b, smem.data());
        else for (long long b = 0; b < blocks(row_items4); ++b) swt_row_fwd4_tile<HLEN, R, NT>(r, b);
        SwtSplitArgs c = k;
        c.in[0] = tmp; c.in[1] = tmp + plane; c.in_bstride = 2 * plane;
        c.out[0] = a.A; c.out[1] = a.H; c.out[2] = a.V; c.out[3] = a.D; c.out_bstride = a.bstride;
        if (colstream && run_swt_colstream<HLEN, false>(c)) return;
        for (long long b = 0; b < blocks(col_items); ++b) swt_col_fwd_tile<HLEN, R, NT>(c, b);
        return;
    }
    SwtSplitArgs c = k;
    c.in[0] = a.A; c.in[1] = a.H; c.in[2] = a.V; c.in[3] = a.D; c.in_bstride = a.bstride; c.out[0] = tmp; c.out_bstride = 2 * plane;
    if (!(colstream && run_swt_colstream<HLEN, true>(c)))
        for (long long b = 0; b < blocks(col_items); ++b) swt_col_inv_tile<HLEN, R, NT>(c, b);
    SwtSplitArgs r = k;
    r.in[0] = tmp; r.in_bstride = 2 * plane; r.out[0] = a.out; r.out_bstride = a.bstride;
    if (f == 1) for (long long b = 0; b < blocks(row_lds); ++b) swt_row_inv_lds_tile<HLEN, 1, 1, NT>(r, b, smem.data());
    else if (f == 2) for (long long b = 0; b < blocks(row_lds); ++b) swt_row_inv_lds_tile<HLEN, 2, 1, NT>(r, b, smem.data());
    else if (f == 4 && !direct) for (long long b = 0; b < blocks(row_lds); ++b) swt_row_inv_lds_tile<HLEN, 4, 1, NT>(r, b, smem.data());
    else for (long long b = 0; b < blocks(row_items4); ++b) swt_row_inv4_tile<HLEN, R, NT>(r, b);
}

EMU_API int emu_swt2_split(int inverse, float* io, int batch, int Nr, int Nc, int level, const float* lo, const float* hi,
                           int hlen, float soft_beta, float* A, float* H, float* V, float* D) {
    Swt2DArgs a;
    a.in = io; a.out = io; a.A = A; a.H = H; a.V = V; a.D = D;
    a.Nr = Nr; a.Nc = Nc; a.f = 1 << (level - 1); a.bstride = (long long)Nr * Nc; a.hlen = hlen; a.soft_beta = soft_beta;
    if ((Nc & 3) || Nc < 16 || a.f >= Nr || a.f >= Nc) return -2;
    set_bank(a.fb, lo, hi, hlen);
    std::vector<float> tmp((size_t)2 * Nr * Nc * batch + (EMU_SLACK ? 16 : 0), NAN);
    switch (hlen) {
#define X(h) case h: run_swt_split<h>(a, batch, inverse != 0, tmp.data()); return 0;
        EMU_SPLIT_HLENS(X)
#undef X
    }
    return -1;
}
