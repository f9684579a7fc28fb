// emu_wave.inc -- the wave-per-tile 2D level kernels and the two-level forward wavefront (dwt2_wave_kernels.hpp).
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).
//
// These kernels stage nothing in LDS.  The two-level forward has an inner function that takes one pointer per plane; its EMU_API
// entry point packs the planes (det1 = H1|V1|D1, band2 = A2|H2|V2|D2) as before and wraps it.

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/dwt2_wave_kernels.hpp"

// the filter lengths that are instantiated (a sanitizer program names fewer: its compile time)
#ifndef EMU_WAVE_HLENS
#define EMU_WAVE_HLENS(X) X(2) X(4) X(6) X(8)
#endif

template <int HLEN>
static void run_fwd_wave(const FwdWaveArgs& a, int batch, int guard) {
    for (int bz = 0; bz < batch; bz++)
        for (int seg = 0; seg < a.segs; seg++)
            for (int strip = 0; strip < a.strips; strip++) {
                if (guard) dwt2_fwd_wave<HLEN, true>(a, strip, seg, bz);
                else dwt2_fwd_wave<HLEN, false>(a, strip, seg, bz);
            }
}

// guard = 0 requires Nc % 256 == 0 and seg_out, Nr2 multiples of GR/2 (checked: returns -2 otherwise)
EMU_API int emu_dwt2_fwd_wave(const float* in, int batch, int Nr, int Nc, const float* lo, const float* hi, int hlen,
                              int seg_out, int guard, float* A, float* H, float* V, float* D) {
    if ((hlen & 1) || hlen < 2 || hlen > 8 || (Nc & 3)) return -1;
    FwdWaveArgs a;
    a.in = in; a.A = A; a.H = H; a.V = V; a.D = D;
    a.Nr = Nr; a.Nc = Nc; a.Nr2 = (Nr + 1) / 2; a.Nc2 = Nc / 2;
    a.in_bstride = (long long)Nr * Nc; a.out_bstride = (long long)a.Nr2 * a.Nc2;
    a.strips = cdiv(Nc, 256); a.seg_out = seg_out; a.segs = cdiv(a.Nr2, seg_out);
    interleave_bank(a.fb, lo, hi, hlen);
    switch (hlen) {
#define X(h) case h: { constexpr int G2 = FwdWaveGeom<h>::GR / 2; \
        if (!guard && ((Nc % 256) || (seg_out % G2) || (a.Nr2 % G2) || (a.Nr2 % seg_out))) return -2; \
        run_fwd_wave<h>(a, batch, guard); return 0; }
        EMU_WAVE_HLENS(X)
#undef X
    }
    return -1;
}

template <int HLEN>
static void run_inv_wave(const InvWaveArgs& a, int batch, int guard) {
    for (int bz = 0; bz < batch; bz++)
        for (int seg = 0; seg < a.segs; seg++)
            for (int strip = 0; strip < a.strips; strip++) {
                if (guard) dwt2_inv_wave<HLEN, true>(a, strip, seg, bz);
                else dwt2_inv_wave<HLEN, false>(a, strip, seg, bz);
            }
}

EMU_API int emu_dwt2_inv_wave(const float* A, const float* H, const float* V, const float* D, int batch, int Nrc, int Ncc,
                              int Nr, int Nc, const float* lo, const float* hi, int hlen, int seg_pairs, int guard,
                              float* out) {
    if ((hlen & 1) || hlen < 2 || hlen > 8 || (Ncc & 1) || Nc != 2 * Ncc) return -1;
    InvWaveArgs a;
    a.A = A; a.H = H; a.V = V; a.D = D; a.out = out;
    a.Nrc = Nrc; a.Ncc = Ncc; a.Nr = Nr; a.Nc = Nc;
    a.in_bstride = (long long)Nrc * Ncc; a.out_bstride = (long long)Nr * Nc;
    a.strips = cdiv(Ncc, 128); a.seg_pairs = seg_pairs; a.segs = cdiv(Nrc, seg_pairs);
    interleave_bank(a.fb, lo, hi, hlen);
    for (int d = 0; d < hlen / 2; d++) {
        a.pl[d].x = lo[hlen - 2 - 2 * d]; a.pl[d].y = lo[hlen - 1 - 2 * d];
        a.ph[d].x = hi[hlen - 2 - 2 * d]; a.ph[d].y = hi[hlen - 1 - 2 * d];
    }
    switch (hlen) {
#define X(h) case h: { constexpr int GRI = InvWaveGeom<h>::GR; \
        if (!guard && ((Ncc % 128) || (seg_pairs % GRI) || (Nrc % GRI) || (Nrc % seg_pairs) || Nr != 2 * Nrc)) return -2; \
        run_inv_wave<h>(a, batch, guard); return 0; }
        EMU_WAVE_HLENS(X)
#undef X
    }
    return -1;
}

// two forward levels per wavefront: in (N0r, N0c) -> l1[3]: H1, V1, D1 (batch x N0r/2 x N0c/2), l2[4]: A2, H2, V2, D2 (batch x N0r/4 x N0c/4)
static int emu_dwt2_fwd2_wave_planes(const float* in, int batch, int N0r, int N0c, const float* lo, const float* hi, int hlen,
                                     int seg2_out, float* const* l1, float* const* l2) {
    if ((hlen & 1) || hlen < 2 || hlen > 8 || (N0r & 3) || (N0c & 15)) return -1;
    FwdWave2Args a;
    a.in = in; a.H1 = l1[0]; a.V1 = l1[1]; a.D1 = l1[2];
    a.A2 = l2[0]; a.H2 = l2[1]; a.V2 = l2[2]; a.D2 = l2[3];
    a.N0r = N0r; a.N0c = N0c;
    a.in_bstride = (long long)N0r * N0c; a.l1_bstride = (long long)(N0r / 2) * (N0c / 2);
    a.l2_bstride = (long long)(N0r / 4) * (N0c / 4);
    a.strips = cdiv(N0c, 240); a.seg2_out = seg2_out; a.segs = cdiv(N0r / 4, seg2_out);
    interleave_bank(a.fb, lo, hi, hlen);
    for (int bz = 0; bz < batch; bz++)
        for (int seg = 0; seg < a.segs; seg++)
            for (int strip = 0; strip < a.strips; strip++) switch (hlen) {
#define X(h) case h: dwt2_fwd2_wave<h>(a, strip, seg, bz); break;
                EMU_WAVE_HLENS(X)
#undef X
                default: return -1;
            }
    return 0;
}

// det1 = H1|V1|D1 planes, band2 = A2|H2|V2|D2 planes
EMU_API int emu_dwt2_fwd2_wave(const float* in, int batch, int N0r, int N0c, const float* lo, const float* hi, int hlen,
                               int seg2_out, float* det1, float* band2) {
    const long long q1 = (long long)batch * (N0r / 2) * (N0c / 2), q2 = (long long)batch * (N0r / 4) * (N0c / 4);
    float* const p1[3] = {det1, det1 + q1, det1 + 2 * q1};
    float* const p2[4] = {band2, band2 + q2, band2 + 2 * q2, band2 + 3 * q2};
    return emu_dwt2_fwd2_wave_planes(in, batch, N0r, N0c, lo, hi, hlen, seg2_out, p1, p2);
}
