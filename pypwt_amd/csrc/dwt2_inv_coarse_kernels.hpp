// dwt2_inv_coarse_kernels.hpp -- the THREE coarsest levels of a large plane undone in one launch (gfx950).
//
// Why: the inverse of one 4096^2 image, four levels, is a chain of dependent launches; its two coarse ones (the two-level
// tile pyramid on levels 4+3 and the level-2 tile launch) move a quarter of the bytes and cost 14.5 of 36 us, each of
// them a latency chain of launch, one load round trip, barrier-separated phases and a store drain.  Every input of an
// inverse exists before the launch, and the synthesis halo does not compound (dwt2_pyramid_kernels.hpp: an inverse
// pyramid workgroup is an ordinary level tile whose A input is synthesised in LDS), so one workgroup can request the
// regions of all ten input planes in ONE round trip and undo three levels out of LDS.
//
// A workgroup is a level-l dwt2_inv_fast_tile (TX x TY coefficients -> 2TY x 2TX samples, inv_fast_col_pass /
// inv_fast_row_pass unchanged: the arithmetic order of the last level is that of the tile kernels).  Its A(l) region
// (R1 x W1 = CR x CXA) is synthesised from an A(l+1) region (R2 x W2), which is synthesised from the four bands of
// level l+2 (R3 x W3).  All regions are compile-time constants relative to the tile's base at their level
// (InvCoarse3Geom); column origins are rounded down to multiples of 4 at every level, so every staged row is whole 16-B
// groups.  db4, 64 x 32 tiles: 37 x 72, 22 x 40 and 14 x 24 coefficients; the two coarse stages add a third of the
// level-l tile's multiply-adds and no bytes that the two launches did not read too.
//
// Loads: one batch of 16-B loads per thread before the first barrier, coarsest level first.  The details of level l -- most
// of the bytes, needed last -- stay in registers while the coarse stages run (the first barrier waits for the coarse loads
// only) and are written to LDS just before the level-l column pass.
//
// LDS: [ (A,V)(l) | (H,D)(l) | tt(l) ] as in dwt2_inv_fast_tile; the coarse regions alias tt, which the level-l column
// pass writes first -- after the last coarse read, with a barrier in between.
//
// The coarse row passes are inv_row_synth4 of the tile kernels: a work item is four adjacent outputs of a row, its window 16-B LDS
// reads issued together, and it writes whole (A,V) pairs -- V of level l+1 from a plain plane staged where tt2 will be, V / H / D of
// level l from the registers of the thread that has held them since phase 1 (the commit is part of the last row pass).
//
// Exactness (as the tile pyramid): values at positions outside a plane are computed from periodically wrapped
// coefficients, which equals the reference's per-level periodization when all three levels have even sizes.  The host
// (launch_dwt2_inv_coarse.hip: dwt2_inv_coarse3_supported) also requires whole 16-B groups per row at all three levels
// and planes at least as large as their staged regions: one conditional add / sub wraps every index.
#pragma once

#include "dwt2_fast_kernels.hpp"

namespace pdwt {

struct InvCoarse3Args {
    const float *A3, *H3, *V3, *D3;  // level l+2: (N0r/8, N0c/8)
    const float *H2, *V2, *D2;       // level l+1: (N0r/4, N0c/4)
    const float *H1, *V1, *D1;       // level l  : (N0r/2, N0c/2)
    float* out;                      // level l-1: (N0r, N0c)
    int N0r, N0c;
    long long l3_bstride, l2_bstride, l1_bstride, out_bstride;
    int tiles_x, tiles_y;            // level-l coefficient tile grid (TX x TY)
    FilterBankI fb;                  // (rec_lo, rec_hi)
    int wt_out = 0;                  // uniform: the output leaves as 16-B write-through stores (launch.hpp: wt_stores_take)
};

constexpr int inv_coarse_floor2(int v) { return v >= 0 ? v / 2 : -((1 - v) / 2); }
constexpr int inv_coarse_floor4(int v) { return v >= 0 ? (v / 4) * 4 : -(((3 - v) / 4) * 4); }

// One synthesis stage seen from its OUTPUT region [O, O + N) (relative to the tile base of the output level): the synthesis
// indices k (output positions 2k - S, 2k + 1 - S) and the input region [I, I + M) relative to the base of the input level
// (half the output's).  QUADS: the input origin rounded down, the extent up, to multiples of 4 (columns).
template <int HLEN, int O, int N, bool QUADS>
struct InvCoarseAxis {
    static constexpr int H2 = HLEN / 2, C = H2 / 2, S = (H2 & 1) ? 0 : 1;
    static constexpr int K_LO = inv_coarse_floor2(O + S), K_HI = inv_coarse_floor2(O + N - 1 + S), NK = K_HI - K_LO + 1;
    static constexpr int I = QUADS ? inv_coarse_floor4(K_LO - C) : K_LO - C;
    static constexpr int M = QUADS ? ((K_HI - C + H2 - I + 3) & ~3) : K_HI - C + H2 - I;
};

template <int HLEN, int TX, int TY>
struct InvCoarse3Geom {
    using G1 = InvFastGeom<HLEN, TX>;
    static constexpr int H2 = G1::H2, C = G1::C, S = G1::S;
    // level l: the region of dwt2_inv_fast_tile, relative to (by TY, bx TX)
    static constexpr int Y1 = -C, R1 = TY + H2 + 1;
    static constexpr int X1 = -C - G1::PADL, W1 = G1::CXA;
    // level l+1, relative to (by TY / 2, bx TX / 2)
    using AY1 = InvCoarseAxis<HLEN, Y1, R1, false>;
    using AX1 = InvCoarseAxis<HLEN, X1, W1, true>;
    static constexpr int Y2 = AY1::I, R2 = AY1::M, X2 = AX1::I, W2 = AX1::M;
    // level l+2, relative to (by TY / 4, bx TX / 4): A(l+1) is synthesised over the whole staged region, alignment columns included
    using AY2 = InvCoarseAxis<HLEN, Y2, R2, false>;
    using AX2 = InvCoarseAxis<HLEN, X2, W2, true>;
    static constexpr int Y3 = AY2::I, R3 = AY2::M, X3 = AX2::I, W3 = AX2::M;
    // LDS, in floats
    static constexpr int BASE = 4 * R1 * W1;                       // (A,V) and (H,D) pairs of level l
    static constexpr int TT = 2 * (2 * TY) * W1;                   // (t1,t2) pairs of level l
    static constexpr int O_AV2 = BASE, O_HD2 = O_AV2 + 2 * R2 * W2, O_TT2 = O_HD2 + 2 * R2 * W2;   // level l+1; tt2: R1 x W2
    static constexpr int O_AV3 = O_TT2 + 2 * R1 * W2, O_HD3 = O_AV3 + 2 * R3 * W3, O_TT3 = O_HD3 + 2 * R3 * W3;  // tt3: R2 x W3
    // (+ 4: the row synthesis reads whole 16-B groups, up to two (t1,t2) pairs past the last one it uses -- behind the last row of tt3)
    static constexpr int COARSE = O_TT3 + 2 * R2 * W3 + 4 - BASE;
    static constexpr int LDS_FLOATS = BASE + (TT > COARSE ? TT : COARSE);
    // the V band of level l+1 waits as a plain R2 x W2 plane where tt2 will be (nobody touches tt2 before the second stage)
    static constexpr int O_V2 = O_TT2;
    static_assert(R2 * W2 <= 2 * R1 * W2, "the plain V plane of level l+1 fits the (t1,t2) plane it borrows");
    static_assert((HLEN & 1) == 0 && HLEN >= 2, "even filters");
    static_assert((TY % 4) == 0 && (TX % 16) == 0, "tile bases are whole samples, and multiples of 4 columns, at all three levels");
    static_assert((X1 & 3) == 0 && (W1 & 3) == 0, "the level-l region is whole 16-B groups");
};

// One synthesis stage out of LDS: the (A,V) / (H,D) pairs of the input region (RI x WI at (YI, XI)) give the A values of the
// output region (RO x WO at (YO, XO)); tt holds RO x WI (t1,t2) pairs in between.  Column pass (inv_coarse_cols), a barrier,
// row pass (inv_coarse_row4 inside inv_coarse_rows / the tile's last stage).
template <int HLEN, int NT, int RI, int WI, int YI, int XI, int RO, int WO, int YO, int XO>
PDWT_DEVICE void inv_coarse_cols(int tid, const v2f* sAVi, const v2f* sHDi, v2f* tti, const FilterBankI& fb) {
    using AY = InvCoarseAxis<HLEN, YO, RO, false>;
    using AX = InvCoarseAxis<HLEN, XO, WO, false>;
    constexpr int H = HLEN, C = AY::C, S = AY::S;
    static_assert(AY::I >= YI && AY::I + AY::M <= YI + RI && AX::I >= XI && AX::I + AX::M <= XI + WI, "the input region covers the stage");
    constexpr int Q2 = WI / 2;
    for (int idx = tid; idx < AY::NK * Q2; idx += NT) {
        const int ki = idx / Q2, q = 2 * (idx - ki * Q2);
        const int kk = AY::K_LO + ki;
        v2f e0, o0, e1, o1;
        inv_col_synth2<H>(&sAVi[(kk - C - YI) * WI + q], &sHDi[(kk - C - YI) * WI + q], WI, fb, e0, o0, e1, o1);
        const int ge = 2 * kk - S - YO, go = ge + 1;  // local output rows
        f32x4 w;
        if (ge >= 0 && ge < RO) {
            w.x = e0.x; w.y = e0.y; w.z = e1.x; w.w = e1.y;
            *reinterpret_cast<f32x4*>(&tti[ge * WI + q]) = w;
        }
        if (go >= 0 && go < RO) {
            w.x = o0.x; w.y = o0.y; w.z = o1.x; w.w = o1.y;
            *reinterpret_cast<f32x4*>(&tti[go * WI + q]) = w;
        }
    }
}

// Row synthesis of a stage, one work item = output row r x output columns 4g .. 4g + 3 (local): inv_row_synth4 on the two
// coefficient columns (XO + 4g) / 2, + 1 of the input level -- the window in 16-B LDS reads issued together, each output summed in
// the order of the tile kernels' row pass.  XO and XI are multiples of 4, so the window's origin has the parity of C and is
// rounded down to an even pair (PE); it may reach up to two pairs past the last one used (InvCoarse3Geom::COARSE has room).
template <int HLEN, int WI, int XI, int XO>
PDWT_DEVICE void inv_coarse_row4(const v2f* tti, int r, int g, const FilterBankI& fb, real_t res[4]) {
    constexpr int C = (HLEN / 2) / 2, PE = C & 1;
    static_assert((XI & 3) == 0 && (XO & 3) == 0 && (WI & 3) == 0, "whole 16-B groups");
    static_assert(XO / 2 - C - XI - PE >= 0, "the window starts inside the staged row");
    const int k = (XO + 4 * g) / 2;  // (a multiple of 4 halved: exact for a negative origin too)
    inv_row_synth4<HLEN, PE>(tti + r * WI + (k - C - XI - PE), fb, res);
}

// ... of a stage whose output level has its V band waiting as a plain RO x WO plane in LDS: whole (A,V) pairs leave as 16-B writes
template <int HLEN, int NT, int WI, int XI, int RO, int WO, int XO>
PDWT_DEVICE void inv_coarse_rows(int tid, const v2f* tti, const real_t* sV, v2f* sAVo, const FilterBankI& fb) {
    constexpr int V4 = WO / 4;
    for (int idx = tid; idx < RO * V4; idx += NT) {
        const int r = idx / V4, g = idx - r * V4;
        real_t res[4];
        inv_coarse_row4<HLEN, WI, XI, XO>(tti, r, g, fb, res);
        const v4f v = lds_load16(sV + r * WO + 4 * g);
        f32x4 w;
        f32x4* d = reinterpret_cast<f32x4*>(sAVo + r * WO + 4 * g);
        w.x = res[0]; w.y = v.x; w.z = res[1]; w.w = v.y; d[0] = w;
        w.x = res[2]; w.y = v.z; w.z = res[3]; w.w = v.w; d[1] = w;
    }
}

// Stage R x W coefficients of up to four planes at (y0, x0) of an (Nr, Nc) level: 16-B loads, a constant number of trips, the
// index clamped (the surplus threads write the last group again, with the same values) and wrapped by one conditional add / sub
// (Nr >= R, Nc >= W, x0 and Nc multiples of 4: a group never straddles the wrap) -- nothing between a thread's loads makes one
// wait for another.  WITH_A: the A plane too, interleaved as in dwt2_inv_fast_tile; otherwise V goes to the plain plane sV (one 16-B
// write per group), where the row pass that synthesises this level's A finds it (inv_coarse_rows).
template <int NT, int R, int W, bool WITH_A>
PDWT_DEVICE void inv_coarse_stage(int tid, const float* PDWT_RESTRICT pA, const float* PDWT_RESTRICT pH, const float* PDWT_RESTRICT pV,
                                  const float* PDWT_RESTRICT pD, long long boff, int y0, int x0, int Nr, int Nc, v2f* sAV, v2f* sHD,
                                  float* sV = nullptr) {
    constexpr int V4 = W / 4, TOTAL = R * V4, TRIPS = (TOTAL + NT - 1) / NT;
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
        int idx = tid + t * NT;
        idx = idx < TOTAL ? idx : TOTAL - 1;
        const int r = idx / V4, g = idx - r * V4;
        int sy = y0 + r, sx = x0 + 4 * g;
        sy = sy < 0 ? sy + Nr : (sy >= Nr ? sy - Nr : sy);
        sx = sx < 0 ? sx + Nc : (sx >= Nc ? sx - Nc : sx);
        const long long o = boff + (long long)sy * Nc + sx;
        const v4f vV = *reinterpret_cast<const v4f*>(pV + o);
        const v4f vH = *reinterpret_cast<const v4f*>(pH + o);
        const v4f vD = *reinterpret_cast<const v4f*>(pD + o);
        if (WITH_A) {
            inv_fast_interleave(sAV, sHD, r * W + 4 * g, *reinterpret_cast<const v4f*>(pA + o), vV, vH, vD);
        } else {
            *reinterpret_cast<v4f*>(sV + r * W + 4 * g) = vV;
            f32x4 w;
            f32x4* dHD = reinterpret_cast<f32x4*>(sHD + r * W + 4 * g);
            w.x = vH.x; w.y = vD.x; w.z = vH.y; w.w = vD.y; dHD[0] = w;
            w.x = vH.z; w.y = vD.z; w.z = vH.w; w.w = vD.w; dHD[1] = w;
        }
    }
}

// The details of level l are the bulk of the bytes and are needed last: their loads are issued with the others, but they stay in
// registers (3 planes x TRIPS groups per thread) while the two coarse stages run, and go to LDS just before the level-l column pass.
template <int NT, int R, int W>
struct InvCoarseHeld {
    static constexpr int V4 = W / 4, TOTAL = R * V4, TRIPS = (TOTAL + NT - 1) / NT;
};

template <int NT, int R, int W>
PDWT_DEVICE void inv_coarse_issue(int tid, const float* PDWT_RESTRICT pH, const float* PDWT_RESTRICT pV, const float* PDWT_RESTRICT pD,
                                  long long boff, int y0, int x0, int Nr, int Nc, v4f* held) {
    using T = InvCoarseHeld<NT, R, W>;
#pragma unroll
    for (int t = 0; t < T::TRIPS; ++t) {
        int idx = tid + t * NT;
        idx = idx < T::TOTAL ? idx : T::TOTAL - 1;
        const int r = idx / T::V4, g = idx - r * T::V4;
        int sy = y0 + r, sx = x0 + 4 * g;
        sy = sy < 0 ? sy + Nr : (sy >= Nr ? sy - Nr : sy);
        sx = sx < 0 ? sx + Nc : (sx >= Nc ? sx - Nc : sx);
        const long long o = boff + (long long)sy * Nc + sx;
        held[3 * t + 0] = *reinterpret_cast<const v4f*>(pV + o);
        held[3 * t + 1] = *reinterpret_cast<const v4f*>(pH + o);
        held[3 * t + 2] = *reinterpret_cast<const v4f*>(pD + o);
    }
}

// The row pass of the LAST stage and the commit in one: a thread's work items are the groups whose level-l details it has held
// since phase 1 -- their A values from inv_coarse_row4, V / H / D from its registers -- so whole (A,V) and (H,D) pairs leave as
// 16-B writes and no A plane waits in LDS for another thread.
template <int HLEN, int NT, int WI, int XI, int R, int W, int XO>
PDWT_DEVICE void inv_coarse_rows_commit(int tid, const v2f* tti, const v4f* held, v2f* sAV, v2f* sHD, const FilterBankI& fb) {
    using T = InvCoarseHeld<NT, R, W>;
#pragma unroll
    for (int t = 0; t < T::TRIPS; ++t) {
        int idx = tid + t * NT;
        idx = idx < T::TOTAL ? idx : T::TOTAL - 1;
        const int r = idx / T::V4, g = idx - r * T::V4;
        real_t res[4];
        inv_coarse_row4<HLEN, WI, XI, XO>(tti, r, g, fb, res);
        const v4f vV = held[3 * t + 0], vH = held[3 * t + 1], vD = held[3 * t + 2];
        f32x4 w;
        f32x4* dAV = reinterpret_cast<f32x4*>(sAV + r * W + 4 * g);
        w.x = res[0]; w.y = vV.x; w.z = res[1]; w.w = vV.y; dAV[0] = w;
        w.x = res[2]; w.y = vV.z; w.z = res[3]; w.w = vV.w; dAV[1] = w;
        f32x4* dHD = reinterpret_cast<f32x4*>(sHD + r * W + 4 * g);
        w.x = vH.x; w.y = vD.x; w.z = vH.y; w.w = vD.y; dHD[0] = w;
        w.x = vH.z; w.y = vD.z; w.z = vH.w; w.w = vD.w; dHD[1] = w;
    }
}

// Requirements (dwt2_inv_coarse3_supported): N0r % 8 == 0, N0c % 32 == 0, N0r >= 8 R3, N0c >= 8 W3 (which bounds the finer
// levels' regions too), 16-B aligned planes and batch strides.
template <int HLEN, int TX, int TY, int NT>
PDWT_DEVICE void dwt2_inv_coarse3_tile(const InvCoarse3Args& a, int bx, int by, int bz, float* smem) {
    using P = InvCoarse3Geom<HLEN, TX, TY>;

    v2f* sAV = reinterpret_cast<v2f*>(smem);  // level l: (A,V), (H,D), then (t1,t2) -- as in dwt2_inv_fast_tile
    v2f* sHD = sAV + P::R1 * P::W1;
    v2f* tt = sHD + P::R1 * P::W1;
    v2f* sAV2 = reinterpret_cast<v2f*>(smem + P::O_AV2);  // the coarse regions alias tt
    v2f* sHD2 = reinterpret_cast<v2f*>(smem + P::O_HD2);
    v2f* tt2 = reinterpret_cast<v2f*>(smem + P::O_TT2);
    float* sV2 = smem + P::O_V2;  // the plain V plane of level l+1, until phase 3 has read it
    v2f* sAV3 = reinterpret_cast<v2f*>(smem + P::O_AV3);
    v2f* sHD3 = reinterpret_cast<v2f*>(smem + P::O_HD3);
    v2f* tt3 = reinterpret_cast<v2f*>(smem + P::O_TT3);

    const int N1r = a.N0r >> 1, N1c = a.N0c >> 1, N2r = a.N0r >> 2, N2c = a.N0c >> 2, N3r = a.N0r >> 3, N3c = a.N0c >> 3;

    // ---- phase 1: the regions of all ten planes, coarsest first (it is needed first), in one batch of loads
    PDWT_PER_THREAD(v4f, held, (3 * InvCoarseHeld<NT, P::R1, P::W1>::TRIPS), NT);
    PDWT_FOR_THREADS(tid, NT) {
        inv_coarse_stage<NT, P::R3, P::W3, true>(tid, a.A3, a.H3, a.V3, a.D3, (long long)bz * a.l3_bstride, by * (TY / 4) + P::Y3,
                                                 bx * (TX / 4) + P::X3, N3r, N3c, sAV3, sHD3);
        inv_coarse_stage<NT, P::R2, P::W2, false>(tid, nullptr, a.H2, a.V2, a.D2, (long long)bz * a.l2_bstride, by * (TY / 2) + P::Y2,
                                                  bx * (TX / 2) + P::X2, N2r, N2c, sAV2, sHD2, sV2);
        inv_coarse_issue<NT, P::R1, P::W1>(tid, a.H1, a.V1, a.D1, (long long)bz * a.l1_bstride, by * TY + P::Y1, bx * TX + P::X1, N1r,
                                           N1c, PDWT_MINE(held, tid));
    }
    PDWT_SYNC();
    // ---- phases 2, 3: level l+2 -> (A,V)(l+1); phases 4, 5: level l+1 -> (A,V)(l), a barrier between every two
    PDWT_FOR_THREADS(tid, NT) {
        inv_coarse_cols<HLEN, NT, P::R3, P::W3, P::Y3, P::X3, P::R2, P::W2, P::Y2, P::X2>(tid, sAV3, sHD3, tt3, a.fb);
    }
    PDWT_SYNC();
    PDWT_FOR_THREADS(tid, NT) { inv_coarse_rows<HLEN, NT, P::W3, P::X3, P::R2, P::W2, P::X2>(tid, tt3, sV2, sAV2, a.fb); }
    PDWT_SYNC();
    PDWT_FOR_THREADS(tid, NT) {  // (tt2 overwrites the plain V plane, which phase 3 has merged into sAV2)
        inv_coarse_cols<HLEN, NT, P::R2, P::W2, P::Y2, P::X2, P::R1, P::W1, P::Y1, P::X1>(tid, sAV2, sHD2, tt2, a.fb);
    }
    PDWT_SYNC();
    // ... with the details of level l, held in registers since phase 1, beside the A values of their own groups
    PDWT_FOR_THREADS(tid, NT) {
        inv_coarse_rows_commit<HLEN, NT, P::W2, P::X2, P::R1, P::W1, P::X1>(tid, tt2, PDWT_MINE(held, tid), sAV, sHD, a.fb);
    }
    PDWT_SYNC();

    // ---- phases 6, 7: the ordinary level-l inverse tile (tt overwrites the coarse regions: nobody reads them any more)
    Inv2DFastArgs f;
    f.A = nullptr; f.H = nullptr; f.V = nullptr; f.D = nullptr;
    f.out = a.out;
    f.Nrc = N1r; f.Ncc = N1c; f.Nr = a.N0r; f.Nc = a.N0c;
    f.in_bstride = a.l1_bstride; f.out_bstride = a.out_bstride;
    f.tiles_x = a.tiles_x; f.tiles_y = a.tiles_y;
    PDWT_FOR_THREADS(tid, NT) { inv_fast_col_pass<HLEN, TX, TY, NT>(tid, sAV, sHD, tt, a.fb); }
    PDWT_SYNC();
    PDWT_FOR_THREADS(tid, NT) {
        f.fb = a.fb;
        inv_fast_row_pass<HLEN, TX, TY, NT>(tid, tt, f, bx, by, bz, a.wt_out != 0);
    }
}

#ifndef PDWT_CPU_EMU
template <int HLEN, int TX, int TY, int NT>
__global__ void __launch_bounds__(NT) dwt2_inv_coarse3_kernel(const InvCoarse3Args a) {
    extern __shared__ __attribute__((aligned(16))) float pdwt_smem[];
    int bx, by;
    if (!xcd_tile(blockIdx.x, a.tiles_x, a.tiles_y, bx, by)) return;
    dwt2_inv_coarse3_tile<HLEN, TX, TY, NT>(a, bx, by, blockIdx.y, pdwt_smem);
}
#endif

}  // namespace pdwt
