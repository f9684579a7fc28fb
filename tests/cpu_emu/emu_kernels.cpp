// CPU emulation build of the gfx950 tile functions (sanitizer / index-math fuzz only).
// Compiles pypwt_amd/csrc/*_kernels.hpp with PDWT_CPU_EMU: phases run as loops over
// thread ids, blocks as loops over the grid.  Test infrastructure; never shipped.
#include "emu_common.hpp"

#include "../../pypwt_amd/csrc/dwt1_fused_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt1_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt1_reg_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt1_rows_kernels.hpp"
#include "../../pypwt_amd/csrc/swt2_fused_kernels.hpp"
#include "../../pypwt_amd/csrc/swt2_fused4_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_fast_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_pyramid_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_pyr3_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_tail_kernels.hpp"
#include "../../pypwt_amd/csrc/swt2_tail_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_strip_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_wave_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_ring_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_long_kernels.hpp"
#include "../../pypwt_amd/csrc/nonsep_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_split_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_colstream_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_fwdstream_kernels.hpp"
#include "../../pypwt_amd/csrc/swt_invstream_kernels.hpp"
#include "../../pypwt_amd/csrc/strip_walk.hpp"
#include "../../pypwt_amd/csrc/swt_stream_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_stream_kernels.hpp"
#include "../../pypwt_amd/csrc/dwt2_split_kernels.hpp"
#include "../../pypwt_amd/csrc/lazy_state.hpp"

template <int HLEN, int TX, int TY, int NT>
static void run_fwd2d(const Fwd2DArgs& a, int batch) {
    std::vector<float> smem(fwd2d_lds_floats<TX, TY>(a.hlen) + 64, -12345.f);
    for (int bz = 0; bz < batch; bz++)
        for (int by = 0; by < cdiv(a.Nr2, TY); by++)
            for (int bx = 0; bx < cdiv(a.Nc2, TX); bx++)
                dwt2_fwd_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
}

template <int HLEN, int TX, int TY, int NT>
static void run_inv2d(const Inv2DArgs& a, int batch) {
    std::vector<float> smem(inv2d_lds_floats<TX, TY>(a.hlen) + 64, -12345.f);
    for (int bz = 0; bz < batch; bz++)
        for (int by = 0; by < cdiv(a.Nr, 2 * TY); by++)
            for (int bx = 0; bx < cdiv(a.Nc, 2 * TX); bx++)
                dwt2_inv_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
}

// generic != 0 forces the runtime-length (HLEN = 0) instantiation
EMU_API int emu_dwt2_fwd(const float* in, int batch, int Nr, int Nc, const float* lo, const float* hi, int hlen,
                         int generic, int tile, float* A, float* H, float* V, float* D) {
    Fwd2DArgs a;
    a.in = in; a.A = A; a.H = H; a.V = V; a.D = D;
    a.Nr = Nr; a.Nc = Nc; a.Nr2 = (Nr + 1) / 2; a.Nc2 = (Nc + 1) / 2;
    a.in_bstride = (long long)Nr * Nc; a.out_bstride = (long long)a.Nr2 * a.Nc2;
    a.hlen = hlen;
    set_bank(a.fb, lo, hi, hlen);
    if (generic || (hlen & 1)) {
        if (tile == 0) run_fwd2d<0, 64, 16, 256>(a, batch); else run_fwd2d<0, 64, 32, 256>(a, batch);
        return 0;
    }
    switch (hlen) {
#define X(h) case h: if (tile == 0) run_fwd2d<h, 64, 16, 256>(a, batch); else run_fwd2d<h, 64, 32, 256>(a, batch); return 0;
        EMU_EVEN_HLENS(X)
#undef X
    }
    return -1;
}

EMU_API int emu_dwt2_inv(const float* A, const float* H, const float* V, const float* D, int batch, int Nrc, int Ncc,
                         int Nr, int Nc, const float* lo, const float* hi, int hlen, int generic, int tile, float* out) {
    Inv2DArgs a;
    a.A = A; a.H = H; a.V = V; a.D = D; a.out = out;
    a.Nrc = Nrc; a.Ncc = Ncc; a.Nr = Nr; a.Nc = Nc;
    a.in_bstride = (long long)Nrc * Ncc; a.out_bstride = (long long)Nr * Nc;
    a.hlen = hlen;
    set_bank(a.fb, lo, hi, hlen);
    if (generic || (hlen & 1)) {
        if (tile == 0) run_inv2d<0, 64, 16, 256>(a, batch); else run_inv2d<0, 64, 32, 256>(a, batch);
        return 0;
    }
    switch (hlen) {
#define X(h) case h: if (tile == 0) run_inv2d<h, 64, 16, 256>(a, batch); else run_inv2d<h, 64, 32, 256>(a, batch); return 0;
        EMU_EVEN_HLENS(X)
#undef X
    }
    return -1;
}

// ------------------------------------------------------------------ 1D DWT
template <int HLEN, int TXO, int NT>
static void run_fwd1d(const Fwd1DArgs& a) {
    std::vector<float> smem(fwd1d_lds_floats<TXO>(a.hlen) + 64, -12345.f);
    for (int row = 0; row < a.rows; row++)
        for (int bx = 0; bx < cdiv(a.Nc2, TXO); bx++) dwt1_fwd_tile<HLEN, TXO, NT>(a, bx, row, smem.data());
}
template <int HLEN, int TXO, int NT>
static void run_inv1d(const Inv1DArgs& a) {
    std::vector<float> smem(inv1d_lds_floats<TXO>(a.hlen) + 64, -12345.f);
    for (int row = 0; row < a.rows; row++)
        for (int bx = 0; bx < cdiv(a.Nc, 2 * TXO); bx++) dwt1_inv_tile<HLEN, TXO, NT>(a, bx, row, smem.data());
}

EMU_API int emu_dwt1_fwd(const float* in, int rows, int Nc, const float* lo, const float* hi, int hlen, int generic,
                         int wide, float* L, float* H) {
    Fwd1DArgs a;
    a.in = in; a.L = L; a.H = H; a.rows = rows; a.Nc = Nc; a.Nc2 = (Nc + 1) / 2; a.hlen = hlen;
    set_bank(a.fb, lo, hi, hlen);
    if (generic || (hlen & 1)) { if (wide) run_fwd1d<0, 1024, 256>(a); else run_fwd1d<0, 256, 256>(a); return 0; }
    switch (hlen) {
#define X(h) case h: if (wide) run_fwd1d<h, 1024, 256>(a); else run_fwd1d<h, 256, 256>(a); return 0;
        EMU_EVEN_HLENS(X)
#undef X
    }
    return -1;
}

EMU_API int emu_dwt1_inv(const float* L, const float* H, int rows, int Ncc, int Nc, const float* lo, const float* hi,
                         int hlen, int generic, int wide, float* out) {
    Inv1DArgs a;
    a.L = L; a.H = H; a.out = out; a.rows = rows; a.Ncc = Ncc; a.Nc = Nc; a.hlen = hlen;
    set_bank(a.fb, lo, hi, hlen);
    if (generic || (hlen & 1)) { if (wide) run_inv1d<0, 1024, 256>(a); else run_inv1d<0, 256, 256>(a); return 0; }
    switch (hlen) {
#define X(h) case h: if (wide) run_inv1d<h, 1024, 256>(a); else run_inv1d<h, 256, 256>(a); return 0;
        EMU_EVEN_HLENS(X)
#undef X
    }
    return -1;
}

// ------------------------------------------------------------------ SWT
template <int HLEN, bool INV>
static void run_swt2(const Swt2DArgs& a, int batch) {
    constexpr int TX = 64, TY = 16, NT = 256;
    std::vector<float> smem(swt2d_lds_floats<TX, TY>(a.hlen) + 64, -12345.f);
    const int M = cdiv(a.Nr, a.f);  // the longest dilation phase (f need not divide Nr)
    for (int bz = 0; bz < batch; bz++)
        for (int by = 0; by < cdiv(M, TY) * a.f; by++)
            for (int bx = 0; bx < cdiv(a.Nc, TX); bx++) {
                if (INV) swt2_inv_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
                else swt2_fwd_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
            }
}

template <int HLEN, bool INV, int TX = 128>
static void run_swt2_vec(const Swt2DArgs& a, int batch) {
    constexpr int TY = 16, NT = 256;
    std::vector<float> smem(swt2d_inv_vec_lds_floats<TX, TY, NT>(HLEN, true) + 64, NAN);
    const int M = cdiv(a.Nr, a.f);  // the longest dilation phase (f need not divide Nr)
    for (int bz = 0; bz < batch; bz++)
        for (int by = 0; by < cdiv(M, TY) * a.f; by++)
            for (int bx = 0; bx < cdiv(a.Nc, TX); bx++) {
                if (INV) swt2_inv_vec_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
                else swt2_fwd_vec_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
            }
}

// inverse != 0: A,H,V,D are inputs and io is the output plane; else io is the input plane
// generic: 0 = compile-time filter length, 1 = run-time filter length, 2 = vectorised (4 columns per thread)
EMU_API int emu_swt2(int inverse, float* io, int batch, int Nr, int Nc, int level, const float* lo, const float* hi,
                     int hlen, int generic, float* A, float* H, float* V, float* D) {
    Swt2DArgs a;
    a.in = io; a.out = io; a.A = A; a.H = H; a.V = V; a.D = D;
    a.Nr = Nr; a.Nc = Nc; a.f = 1 << (level - 1); a.bstride = (long long)Nr * Nc; a.hlen = hlen; a.soft_beta = 0.f;
    set_bank(a.fb, lo, hi, hlen);
    if (generic == 3) {  // the 256-column tiles the host uses for hlen 2 and 4
        if (Nc < 4 || (hlen != 2 && hlen != 4)) return -3;
        if (hlen == 2) { if (inverse) run_swt2_vec<2, true, 256>(a, batch); else run_swt2_vec<2, false, 256>(a, batch); }
        else { if (inverse) run_swt2_vec<4, true, 256>(a, batch); else run_swt2_vec<4, false, 256>(a, batch); }
        return 0;
    }
    if (generic == 2) {
        if ((hlen & 1) || Nc < 4) return -3;  // rows of any length (round 5)
        switch (hlen) {
#define X(h) case h: if (inverse) run_swt2_vec<h, true>(a, batch); else run_swt2_vec<h, false>(a, batch); return 0;
            EMU_EVEN_HLENS(X)
#undef X
        }
        return -1;
    }
    if (generic || (hlen & 1)) { if (inverse) run_swt2<0, true>(a, batch); else run_swt2<0, false>(a, batch); return 0; }
    switch (hlen) {
#define X(h) case h: if (inverse) run_swt2<h, true>(a, batch); else run_swt2<h, false>(a, batch); return 0;
        EMU_EVEN_HLENS(X)
#undef X
    }
    return -1;
}

EMU_API int emu_swt_pass(int inverse, const float* in0, const float* in1, int Nr, int Nc, int level, int along_y,
                         const float* lo, const float* hi, int hlen, float* out0, float* out1) {
    SwtPassArgs a;
    a.in0 = in0; a.in1 = in1; a.out0 = out0; a.out1 = out1;
    a.Nr = Nr; a.Nc = Nc; a.f = 1 << (level - 1); a.along_y = along_y; a.hlen = hlen;
    set_bank(a.fb, lo, hi, hlen);
    const long long total = (long long)Nr * Nc;
    for (long long b = 0; b < (total + 255) / 256; b++) {
        if (inverse) swt_pass_inv_tile<256>(a, b, nullptr);
        else swt_pass_fwd_tile<256>(a, b, nullptr);
    }
    return 0;
}

// ------------------------------------------------------------------ tuned 2D kernels
#include "emu_dwt2_fast.inc"

// ------------------------------------------------------------------ non-separable
// filt: 4 banks of hlen*hlen ; inverse != 0: A..D inputs, io output
EMU_API int emu_nonsep(int inverse, float* io, int batch, int Nr, int Nc, int do_swt, int level, const float* filt,
                       int hlen, float* A, float* H, float* V, float* D) {
    NonsepArgs a;
    a.in = io; a.out = io; a.A = A; a.H = H; a.V = V; a.D = D; a.filt = filt;
    a.Nr = Nr; a.Nc = Nc; a.Nrc = do_swt ? Nr : (Nr + 1) / 2; a.Ncc = do_swt ? Nc : (Nc + 1) / 2;
    a.f = 1 << (level - 1); a.do_swt = do_swt;
    a.img_bstride = (long long)Nr * Nc; a.coef_bstride = (long long)a.Nrc * a.Ncc; a.hlen = hlen;
    std::vector<float> smem(nonsep_lds_floats(hlen) + 16, -1.f);
    const long long total = inverse ? (long long)Nr * Nc : (long long)a.Nrc * a.Ncc;
    for (int bz = 0; bz < batch; bz++)
        for (long long b = 0; b < (total + 255) / 256; b++) {
            if (inverse) nonsep_inv_tile<256>(a, b, bz, smem.data());
            else nonsep_fwd_tile<256>(a, b, bz, smem.data());
        }
    return 0;
}

// ------------------------------------------------------------------ fused multi-level 1D
#include "emu_dwt1_fused.inc"

// ------------------------------------------------------------------ two- and three-level pyramids
#include "emu_pyramid.inc"

// ------------------------------------------------------------------ whole transforms in one workgroup: 2D tail, rows tail, SWT tail
#include "emu_tail.inc"

// ------------------------------------------------------------------ two-level streaming strips (forward)
template <int HLEN, int TX2, int NT>
static void run_fwd_strip2(FwdStrip2Args a, int batch) {
    std::vector<float> smem(Strip2Geom<HLEN, TX2>::LDS_FLOATS + 64, NAN);
    a.strips = cdiv(a.N0c / 4, TX2); a.segs = cdiv(a.N0r / 4, a.seg2);
    for (int bz = 0; bz < batch; bz++)
        for (int sg = 0; sg < a.segs; sg++)
            for (int st = 0; st < a.strips; st++) dwt2_fwd_strip2_wg<HLEN, TX2, NT>(a, st, sg, bz, smem.data());
}

EMU_API int emu_dwt2_fwd_strip2(const float* in, int batch, int N0r, int N0c, const float* lo, const float* hi, int hlen,
                                int seg2, float* l1, float* l2) {
    if ((hlen & 1) || hlen > 8 || (N0c & 7) || (N0r & 3)) return -2;
    FwdStrip2Args a;
    const long long n1 = (long long)batch * (N0r / 2) * (N0c / 2), n2 = (long long)batch * (N0r / 4) * (N0c / 4);
    a.in = in; a.H1 = l1; a.V1 = l1 + n1; a.D1 = l1 + 2 * n1;
    a.A2 = l2; a.H2 = l2 + n2; a.V2 = l2 + 2 * n2; a.D2 = l2 + 3 * n2;
    a.N0r = N0r; a.N0c = N0c; a.seg2 = seg2;
    a.in_bstride = (long long)N0r * N0c; a.l1_bstride = (long long)(N0r / 2) * (N0c / 2);
    a.l2_bstride = (long long)(N0r / 4) * (N0c / 4);
    set_bank_i(a.fb, lo, hi, hlen);
    switch (hlen) {
#define X(h) case h: run_fwd_strip2<h, 32, 256>(a, batch); return 0;
        X(2) X(4) X(6) X(8)
#undef X
    }
    return -1;
}

template <int HLEN, int TX, int NT>
static void run_inv_strip2(InvStrip2Args a, int batch) {
    std::vector<float> smem(InvStrip2Geom<HLEN, TX>::LDS_FLOATS + 64, NAN);
    a.strips = cdiv(a.N0c / 2, TX); a.segs = cdiv(a.N0r, a.seg_rows);
    for (int bz = 0; bz < batch; bz++)
        for (int sg = 0; sg < a.segs; sg++)
            for (int st = 0; st < a.strips; st++) dwt2_inv_strip2_wg<HLEN, TX, NT>(a, st, sg, bz, smem.data());
}

EMU_API int emu_dwt2_inv_strip2(const float* l1, const float* l2, int batch, int N0r, int N0c, const float* lo,
                                const float* hi, int hlen, int seg_rows, float* out) {
    if ((hlen & 1) || hlen > 8 || (N0c & 15) || (N0r & 3)) return -2;
    InvStrip2Args a;
    const long long n1 = (long long)batch * (N0r / 2) * (N0c / 2), n2 = (long long)batch * (N0r / 4) * (N0c / 4);
    a.H1 = l1; a.V1 = l1 + n1; a.D1 = l1 + 2 * n1;
    a.A2 = l2; a.H2 = l2 + n2; a.V2 = l2 + 2 * n2; a.D2 = l2 + 3 * n2;
    a.out = out; a.N0r = N0r; a.N0c = N0c; a.seg_rows = seg_rows;
    a.out_bstride = (long long)N0r * N0c; a.l1_bstride = (long long)(N0r / 2) * (N0c / 2);
    a.l2_bstride = (long long)(N0r / 4) * (N0c / 4);
    set_bank_i(a.fb, lo, hi, hlen);
    switch (hlen) {
#define X(h) case h: run_inv_strip2<h, 64, 256>(a, batch); return 0;
        X(2) X(4) X(6) X(8)
#undef X
    }
    return -1;
}

// ------------------------------------------------------------------ wave-per-tile 2D level kernels, two forward levels per wavefront
#include "emu_wave.inc"

// ------------------------------------------------------------------ register-ring level kernels for long filters
#include "emu_ring.inc"

// ------------------------------------------------------------------ 1D, up to three levels in registers
#include "emu_dwt1_reg.inc"

#include "emu_swt_fused.inc"

// ---- host-side geometry of the strip walks and of the any-size fused groups (pure functions)
EMU_API int emu_strip_walk_seg(int rows, long long units, int ty, int warm, int slots) { return strip_walk_seg(rows, units, ty, warm, slots); }
EMU_API int emu_swt_stage_pad(int x0, int xs, int Nc) { return swt_stage_pad(x0, xs, Nc); }
// the source column of group g of the (xs + 6) / 4 groups the one-launch SWT kernels load per staged row of the window [x0, x0 + xs)
EMU_API int emu_swt_stage_col(int x0, int xs, int Nc, int g) { return swt_stage_col(x0, swt_stage_pad(x0, xs, Nc), xs, g, Nc); }
EMU_API void emu_swt_walk(int Nr, int Nc, int f0, int cols_per_lane, int* out4) {
    const SwtWalk w = swt_walk(Nr, Nc, f0, cols_per_lane);
    out4[0] = w.phases; out4[1] = w.rows_phase; out4[2] = (int)w.magic; out4[3] = w.pad;
}
EMU_API int emu_swt_walk_row(int Nr, int Nc, int f0, int py, int idx) {
    const SwtWalk w = swt_walk(Nr, Nc, f0, 4);
    return swt_walk_row<true, 1>(w, Nr, py, idx * f0);
}

#include "emu_swt_fwdstream.inc"

#include "emu_swt_invstream.inc"

#include "emu_swt_split.inc"  // (with the column pass as a strip walk)

// ---- the a-trous row kernels as the (batched) 1D transform
#include "emu_swt_rows.inc"

// ---- one DECIMATED level as a row pass + a column pass through scratch (dwt2_split_kernels.hpp).  forward: in (Nr, Nc) ->
// A, H, V, D (Nr/2, Nc/2); inverse: A, H, V, D -> io (Nr, Nc).  R = output rows per work item of the column kernels.
template <int HLEN, int R>
static void run_dwt_split(bool inverse, float* io, int batch, int Nr, int Nc, const FilterBank& fb, float* A, float* H, float* V,
                          float* D, float* tmp) {
    constexpr int NT = 256;
    const int Nr2 = Nr / 2, Nc2 = Nc / 2;
    DwtSplitArgs k{};
    k.batch = batch;
    for (int j = 0; j < HLEN; ++j) k.t.t[j] = mk2(fb.lo[HLEN - 1 - j], fb.hi[HLEN - 1 - j]);
    std::vector<float> smem(16384, NAN);  // one workgroup's LDS
    auto blocks = [](long long waves) { return (waves + NT / 64 - 1) / (NT / 64); };
    const long long img = (long long)Nr * Nc, band = (long long)Nr2 * Nc2;
    if (!inverse) {
        const long long plane = (long long)Nr * Nc2;
        DwtSplitArgs r = k;
        r.rows = Nr; r.cols = Nc; r.in[0] = io; r.in_bstride = img;
        r.out[0] = tmp; r.out[1] = tmp + plane; r.out_bstride = 2 * plane;
        for (long long b = 0; b < blocks(dwt_row_waves(batch, Nr, Nc)); ++b) dwt_row_fwd_tile<HLEN, NT>(r, b, smem.data());
        DwtSplitArgs c = k;
        c.rows = Nr; c.cols = Nc2; c.in[0] = tmp; c.in[1] = tmp + plane; c.in_bstride = 2 * plane;
        c.out[0] = A; c.out[1] = H; c.out[2] = V; c.out[3] = D; c.out_bstride = band;
        for (long long b = 0; b < blocks(dwt_col_waves(batch, Nr2, Nc2, R)); ++b) dwt_col_fwd_tile<HLEN, R, NT, (R == 4 ? 8 : 2)>(c, b);
        return;
    }
    DwtSplitArgs c = k;
    c.rows = Nr2; c.cols = Nc2; c.in[0] = A; c.in[1] = H; c.in[2] = V; c.in[3] = D; c.in_bstride = band;
    c.out[0] = tmp; c.out_bstride = img;
    for (long long b = 0; b < blocks(dwt_col_waves(batch, Nr, Nc2, R)); ++b) dwt_col_inv_tile<HLEN, R, NT, (R == 4 ? 4 : (R == 2 ? 3 : 2))>(c, b);
    DwtSplitArgs r = k;
    r.rows = Nr; r.cols = Nc2; r.in[0] = tmp; r.in_bstride = img; r.out[0] = io; r.out_bstride = img;
    for (long long b = 0; b < blocks(dwt_row_waves(batch, Nr, Nc)); ++b) dwt_row_inv_tile<HLEN, NT>(r, b, smem.data());
}

EMU_API int emu_dwt2_split(int inverse, float* io, int batch, int Nr, int Nc, const float* lo, const float* hi, int hlen, int R,
                           float* A, float* H, float* V, float* D) {
    if ((Nr & 1) || (Nc & 7) || Nc < 16) return -2;
    FilterBank fb;
    set_bank(fb, lo, hi, hlen);
    std::vector<float> tmp((size_t)Nr * Nc * batch + 16, NAN);
    switch (hlen) {
#define X(h)                                                                                              \
    case h:                                                                                               \
        if (R == 2) run_dwt_split<h, 2>(inverse != 0, io, batch, Nr, Nc, fb, A, H, V, D, tmp.data());      \
        else if (R == 4) run_dwt_split<h, 4>(inverse != 0, io, batch, Nr, Nc, fb, A, H, V, D, tmp.data()); \
        else run_dwt_split<h, 8>(inverse != 0, io, batch, Nr, Nc, fb, A, H, V, D, tmp.data());             \
        return 0;
        X(10) X(12) X(14) X(16) X(20) X(22) X(26) X(38) X(40)
#undef X
    }
    return -1;
}


// ---- one level, a-trous or decimated, as two launches of the any-length stream kernels
#include "emu_stream.inc"

#include "emu_dwt2_long.inc"

// one row of the lazy-state table (lazy_state.hpp): {refuses after inverse(), what becomes of a pending threshold, of a consumed one};
// -1 past the last Entry
EMU_API int emu_lazy_row(int entry, int* out3) {
    if (entry < 0 || entry >= (int)pdwt::Entry::count_) return -1;
    const pdwt::LazyRow r = pdwt::lazy_row((pdwt::Entry)entry);
    out3[0] = r.refuses_after_inverse;
    out3[1] = (int)r.pending;
    out3[2] = (int)r.consumed;
    return 0;
}
