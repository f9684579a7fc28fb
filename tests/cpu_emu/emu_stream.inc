// emu_stream.inc -- one level as two launches of the any-length stream kernels: the a-trous level (swt_stream_kernels.hpp) and the
// decimated level (dwt2_stream_kernels.hpp), the fp64 library's long filters.
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).
//
// These kernels stage nothing in LDS.  The two intermediate planes between the launches are two blocks of exactly batch images each
// (plus EMU_SLACK elements), not one packed allocation: a read behind the first does not land in the second.

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/swt_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_stream_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_stream_kernels.hpp"

// ---- one a-trous level; planes as in emu_swt2.  nc = columns per work item (2: pairs where rows are even), R = outputs per work item
template <int NC, int R>
static void run_swt_stream(const Swt2DArgs& a, int batch, bool inverse, float* tmp0, float* tmp1) {
    constexpr int NT = 256;
    const long long plane = (long long)a.Nr * a.Nc;
    SwtStreamArgs k{};
    k.Nr = a.Nr; k.Nc = a.Nc; k.f = a.f; k.batch = batch; k.hlen = a.hlen; k.scale = 0.5f;
    for (int j = 0; j < a.hlen; ++j) {
        k.tl[kStreamPadL + j] = a.fb.lo[a.hlen - 1 - j];
        k.th[kStreamPadL + j] = a.fb.hi[a.hlen - 1 - j];
    }
    auto blocks = [](long long waves) { return (waves + NT / 64 - 1) / (NT / 64); };
    auto rows = [&](const SwtStreamArgs& r, bool syn) {
        const bool two = NC == 2 && !(a.f & 1);
        const long long n = blocks(stream_waves_x(r.problems, batch, a.Nr, a.Nc, a.f, R, two ? 2 : 1));
        for (long long b = 0; b < n; ++b) {
            if (syn) { if (two) swt_stream_tile<true, false, NC, R, NT>(r, b); else swt_stream_tile<true, false, 1, R, NT>(r, b); }
            else { if (two) swt_stream_tile<false, false, NC, R, NT>(r, b); else swt_stream_tile<false, false, 1, R, NT>(r, b); }
        }
    };
    auto cols = [&](const SwtStreamArgs& c, bool syn) {
        const long long n = blocks(stream_waves_y(c.problems, batch, a.Nr, a.Nc, a.f, R, NC));
        for (long long b = 0; b < n; ++b) {
            if (syn) swt_stream_tile<true, true, NC, R, NT>(c, b);
            else swt_stream_tile<false, true, NC, R, NT>(c, b);
        }
    };
    if (!inverse) {
        SwtStreamArgs r = k;
        r.problems = 1; r.in[0][0] = a.in; r.in_bstride = a.bstride;
        r.out[0][0] = tmp0; r.out[0][1] = tmp1; r.out_bstride = plane;
        rows(r, false);
        SwtStreamArgs c = k;
        c.problems = 2; c.in[0][0] = tmp0; c.in[1][0] = tmp1; c.in_bstride = plane;
        c.out[0][0] = a.A; c.out[0][1] = a.H; c.out[1][0] = a.V; c.out[1][1] = a.D; c.out_bstride = a.bstride;
        cols(c, false);
        return;
    }
    SwtStreamArgs c = k;
    c.problems = 2; c.in[0][0] = a.A; c.in[0][1] = a.H; c.in[1][0] = a.V; c.in[1][1] = a.D; c.in_bstride = a.bstride;
    c.soft[0][1] = c.soft[1][0] = c.soft[1][1] = a.soft_beta;
    c.out[0][0] = tmp0; c.out[1][0] = tmp1; c.out_bstride = plane;
    cols(c, true);
    SwtStreamArgs r = k;
    r.problems = 1; r.in[0][0] = tmp0; r.in[0][1] = tmp1; r.in_bstride = plane;
    r.out[0][0] = a.out; r.out_bstride = a.bstride;
    rows(r, true);
}

EMU_API int emu_swt2_stream(int inverse, float* io, int batch, int Nr, int Nc, int level, const float* lo, const float* hi,
                            int hlen, float soft_beta, float* A, float* H, float* V, float* D, int R) {
    Swt2DArgs a;
    a.in = io; a.out = io; a.A = A; a.H = H; a.V = V; a.D = D;
    a.Nr = Nr; a.Nc = Nc; a.f = 1 << (level - 1); a.bstride = (long long)Nr * Nc; a.hlen = hlen; a.soft_beta = soft_beta;
    if (a.f >= Nr || a.f >= Nc || hlen > kMaxTaps) return -2;
    set_bank(a.fb, lo, hi, hlen);
    std::vector<float> tmp0((size_t)Nr * Nc * batch + EMU_SLACK, NAN), tmp1((size_t)Nr * Nc * batch + EMU_SLACK, NAN);
    const bool two = !(Nc & 1);  // (the emulation's planes are 8-B aligned floats: pairs need even rows only)
    if (R == 4) { if (two) run_swt_stream<2, 4>(a, batch, inverse != 0, tmp0.data(), tmp1.data()); else run_swt_stream<1, 4>(a, batch, inverse != 0, tmp0.data(), tmp1.data()); }
    else if (R == 8) { if (two) run_swt_stream<2, 8>(a, batch, inverse != 0, tmp0.data(), tmp1.data()); else run_swt_stream<1, 8>(a, batch, inverse != 0, tmp0.data(), tmp1.data()); }
    else if (R == 2) { if (two) run_swt_stream<2, 2>(a, batch, inverse != 0, tmp0.data(), tmp1.data()); else run_swt_stream<1, 2>(a, batch, inverse != 0, tmp0.data(), tmp1.data()); }
    else return -1;
    return 0;
}

// ---- one DECIMATED level; forward: in (Nr, Nc) -> A, H, V, D (Nr/2, Nc/2); inverse: A, H, V, D -> io (Nr, Nc).  Even sizes, even
// filter lengths.
template <int NC, int R>
static void run_dwt_stream(bool inverse, float* io, int batch, int Nr, int Nc, const FilterBank& fb, int hlen, float* A, float* H, float* V,
                           float* D, float* tmp0, float* tmp1) {
    constexpr int NT = 256;
    const int Nr2 = Nr / 2, Nc2 = Nc / 2;
    const long long plane = (long long)Nr * Nc2, img = (long long)Nr * Nc, band = (long long)Nr2 * Nc2;
    DwtStreamArgs k{};
    k.batch = batch; k.hlen = hlen;
    if (!inverse) {
        for (int j = 0; j < hlen; ++j) { k.t[0][kStreamPadL + j] = fb.lo[hlen - 1 - j]; k.t[1][kStreamPadL + j] = fb.hi[hlen - 1 - j]; }
    } else {
        for (int j = 0; j < hlen / 2; ++j)
            for (int par = 0; par < 2; ++par) {
                k.t[par][kStreamPadL + j] = fb.lo[hlen - 1 - (2 * j + 1 - par)];
                k.t[2 + par][kStreamPadL + j] = fb.hi[hlen - 1 - (2 * j + 1 - par)];
            }
    }
    auto blocks = [](long long waves) { return (waves + NT / 64 - 1) / (NT / 64); };
    if (!inverse) {
        DwtStreamArgs r = k;
        r.problems = 1; r.in_rows = Nr; r.in_cols = Nc; r.out_rows = Nr; r.out_cols = Nc2;
        r.in[0][0] = io; r.in_bstride = img; r.out[0][0] = tmp0; r.out[0][1] = tmp1; r.out_bstride = plane;
        for (long long b = 0; b < blocks(dwt_stream_waves(false, 1, batch, Nr, Nc, Nc2, R, 1)); ++b) dwt_stream_tile<false, false, 1, R, NT>(r, b);
        DwtStreamArgs c = k;
        c.problems = 2; c.in_rows = Nr; c.in_cols = Nc2; c.out_rows = Nr2; c.out_cols = Nc2;
        c.in[0][0] = tmp0; c.in[1][0] = tmp1; c.in_bstride = plane;
        c.out[0][0] = A; c.out[0][1] = H; c.out[1][0] = V; c.out[1][1] = D; c.out_bstride = band;
        for (long long b = 0; b < blocks(dwt_stream_waves(true, 2, batch, Nr, Nc2, Nr2, R, NC)); ++b) dwt_stream_tile<false, true, NC, R, NT>(c, b);
        return;
    }
    DwtStreamArgs c = k;
    c.problems = 2; c.in_rows = Nr2; c.in_cols = Nc2; c.out_rows = Nr; c.out_cols = Nc2;
    c.in[0][0] = A; c.in[0][1] = H; c.in[1][0] = V; c.in[1][1] = D; c.in_bstride = band;
    c.out[0][0] = tmp0; c.out[1][0] = tmp1; c.out_bstride = plane;
    for (long long b = 0; b < blocks(dwt_stream_waves(true, 2, batch, Nr2, Nc2, Nr2, R, NC)); ++b) dwt_stream_tile<true, true, NC, R, NT>(c, b);
    DwtStreamArgs r = k;
    r.problems = 1; r.in_rows = Nr; r.in_cols = Nc2; r.out_rows = Nr; r.out_cols = Nc;
    r.in[0][0] = tmp0; r.in[0][1] = tmp1; r.in_bstride = plane; r.out[0][0] = io; r.out_bstride = img;
    for (long long b = 0; b < blocks(dwt_stream_waves(false, 1, batch, Nr, Nc2, Nc2, R, 1)); ++b) dwt_stream_tile<true, false, 1, R, NT>(r, b);
}

EMU_API int emu_dwt2_stream(int inverse, float* io, int batch, int Nr, int Nc, const float* lo, const float* hi, int hlen, int R,
                            float* A, float* H, float* V, float* D) {
    if ((Nr & 1) || (Nc & 1) || (hlen & 1) || hlen > kMaxTaps) return -2;
    FilterBank fb;
    set_bank(fb, lo, hi, hlen);
    // the two half-width planes between the launches (batch x Nr x Nc/2 each)
    std::vector<float> tmp0((size_t)Nr * (Nc / 2) * batch + EMU_SLACK, NAN), tmp1((size_t)Nr * (Nc / 2) * batch + EMU_SLACK, NAN);
    const bool two = !((Nc / 2) & 1);
    if (R == 4) { if (two) run_dwt_stream<2, 4>(inverse != 0, io, batch, Nr, Nc, fb, hlen, A, H, V, D, tmp0.data(), tmp1.data()); else run_dwt_stream<1, 4>(inverse != 0, io, batch, Nr, Nc, fb, hlen, A, H, V, D, tmp0.data(), tmp1.data()); }
    else if (R == 2) { if (two) run_dwt_stream<2, 2>(inverse != 0, io, batch, Nr, Nc, fb, hlen, A, H, V, D, tmp0.data(), tmp1.data()); else run_dwt_stream<1, 2>(inverse != 0, io, batch, Nr, Nc, fb, hlen, A, H, V, D, tmp0.data(), tmp1.data()); }
    else return -1;
    return 0;
}
