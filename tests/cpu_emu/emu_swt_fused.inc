// emu_swt_fused.inc -- 2-tap and 4-tap SWT groups of levels in one launch (swt2_fused_kernels.hpp, swt2_fused4_kernels.hpp).
// Part of the CPU emulation of the tile functions: included by emu_kernels.cpp (the shared library of tests/emu_util.py) and, on its own,
// by emu_san.cpp (a stand-alone program per kernel family for the address and undefined-behaviour sanitizers).

#pragma once
#include "emu_common.hpp"
#include "../../pypwt_amd/csrc/swt2_fused_kernels.hpp"
#include "../../pypwt_amd/csrc/swt2_fused4_kernels.hpp"

// ------------------------------------------------------------------ 2D SWT, 2-tap filters, two or three levels per launch
template <int K, int F0>
static void run_swt_fused(SwtFusedArgs& a, int batch, bool inverse, int cpl) {
    // sizes the aligned instantiations cannot take run the GEN ones (SwtWalk); `cpl` + 8 forces them on every size
    const bool gen = swt_walk_general(a.Nr, a.Nc, F0) || cpl >= 8;
    cpl &= 7;
    a.wk = swt_walk(a.Nr, a.Nc, F0, inverse ? cpl : 4);
    if (inverse) a.strips = cpl == 2 ? swt_walk_strips(a.wk, a.Nc, 2 * SwtInvGeom<K, F0, 2>::V) : swt_walk_strips(a.wk, a.Nc, 4 * SwtInvGeom<K, F0, 4>::V);
    else a.strips = swt_walk_strips(a.wk, a.Nc, 4 * SwtFusedGeom<K, F0>::V);
    a.segs = (a.wk.rows_phase + a.seg_rows - 1) / a.seg_rows;
    const long long waves = (long long)batch * a.wk.phases * a.segs * a.strips;
    for (long long w = 0; w < waves; w++) {
        if (!inverse) { if (gen) swt2_fwd_fused<K, F0, true>(a, w); else swt2_fwd_fused<K, F0, false>(a, w); }
        else if (cpl == 2) { if (gen) swt2_inv_fused<K, F0, 4, 2, true>(a, w); else swt2_inv_fused<K, F0, 4, 2, false>(a, w); }
        else { if (gen) swt2_inv_fused<K, F0, 4, 4, true>(a, w); else swt2_inv_fused<K, F0, 4, 4, false>(a, w); }
    }
}

// planes: forward  in -> det (K x [H, V, D] planes, level l0 first) and out;  inverse  in (A) + det -> out
EMU_API int emu_swt2_fused(const float* in, float* det, float* out, int batch, int Nr, int Nc, int K, int f0, int seg_rows,
                           const float* lo, const float* hi, const float* beta, int inverse, int cpl) {
    if (K < 2 || K > 3 || (f0 != 1 && f0 != 8) || Nc < 256 || Nr / f0 < (1 << K) || seg_rows % (1 << K)) return -2;
    SwtFusedArgs a;
    const long long plane = (long long)Nr * Nc;
    a.in = in; a.out = out; a.Nr = Nr; a.Nc = Nc; a.bstride = plane;
    for (int k = 0; k < kSwtFusedMaxLevels; k++) {
        a.H[k] = a.V[k] = a.D[k] = nullptr;
        a.beta[k] = (beta && k < K) ? beta[k] : 0.f;
    }
    for (int k = 0; k < K; k++) {
        a.H[k] = det + (3 * k + 0) * batch * plane;
        a.V[k] = det + (3 * k + 1) * batch * plane;
        a.D[k] = det + (3 * k + 2) * batch * plane;
    }
    a.lo[0] = lo[0]; a.lo[1] = lo[1]; a.hi[0] = hi[0]; a.hi[1] = hi[1];
    a.seg_rows = seg_rows;
    a.segs = (Nr / f0 + seg_rows - 1) / seg_rows;
#define Y(k, f) if (K == k && f0 == f) { run_swt_fused<k, f>(a, batch, inverse != 0, cpl); return 0; }
    Y(2, 1) Y(3, 1) Y(2, 8) Y(3, 8)
#undef Y
    return -1;
}

// ---- 4-tap fused SWT pairs (swt2_fused4_kernels.hpp): planes as in emu_swt2_fused with K = 2
template <int F0>
static void run_swt4(Swt4Args& a, int batch, bool inverse, bool gen) {
    using G = Swt4Geom<F0>;
    const int V = inverse ? G::Vi : G::Vf;
    a.wk = swt_walk(a.Nr, a.Nc, F0, 4);
    a.strips = swt_walk_strips(a.wk, a.Nc, 4 * V);
    a.segs = (a.wk.rows_phase + a.seg_rows - 1) / a.seg_rows;
    const long long waves = (long long)batch * a.wk.phases * a.segs * a.strips;
    for (long long w = 0; w < waves; w++) {
        if (!inverse) { if (gen) swt4_fwd_fused<F0, true>(a, w); else swt4_fwd_fused<F0, false>(a, w); }
        else { if (gen) swt4_inv_fused<F0, 4, true>(a, w); else swt4_inv_fused<F0, 4, false>(a, w); }
    }
}

EMU_API int emu_swt4_fused(const float* in, float* det, float* out, int batch, int Nr, int Nc, int f0, int seg_rows,
                           const float* lo, const float* hi, const float* beta, int inverse) {
    const bool gen = swt_walk_general(Nr, Nc, f0) || (inverse & 2);  // inverse + 2: the GEN instantiations on every size
    if ((f0 != 1 && f0 != 4) || Nc < (gen ? 256 : 64) || Nr / f0 < 8 || seg_rows % 8) return -2;
    Swt4Args a;
    const long long plane = (long long)Nr * Nc;
    a.in = in; a.out = out; a.Nr = Nr; a.Nc = Nc; a.bstride = plane;
    for (int k = 0; k < 2; k++) {
        a.H[k] = det + (3 * k + 0) * batch * plane;
        a.V[k] = det + (3 * k + 1) * batch * plane;
        a.D[k] = det + (3 * k + 2) * batch * plane;
        a.beta[k] = beta ? beta[k] : 0.f;
    }
    for (int j = 0; j < 4; j++) { a.lo[j] = lo[j]; a.hi[j] = hi[j]; }
    a.seg_rows = seg_rows;
    a.segs = (Nr / f0 + seg_rows - 1) / seg_rows;
    if (f0 == 1) run_swt4<1>(a, batch, (inverse & 1) != 0, gen);
    else run_swt4<4>(a, batch, (inverse & 1) != 0, gen);
    return 0;
}
