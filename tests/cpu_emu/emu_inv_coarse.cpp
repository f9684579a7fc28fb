// CPU emulation of dwt2_inv_coarse3_tile (pypwt_amd/csrc/dwt2_inv_coarse_kernels.hpp): the tile function compiled with g++
// (-DPDWT_CPU_EMU: a phase is a loop over thread ids, a barrier nothing), every candidate tile shape of
// launch_dwt2_inv_coarse.hip.  tests/test_emu_inv_coarse.py builds it as a shared library and compares with the oracle;
// with -DEMU_INV_COARSE_MAIN it is a stand-alone program for a sanitizer build (-fsanitize=address,undefined): it runs
// every shape and filter length over planes with interior, border and partial tiles and checks each result against a
// level-by-level synthesis written out plainly below.  The emulated LDS is sized exactly and starts as NaN: a read of
// anything that was not written shows in the output, a read past the end to the sanitizer.
#define PDWT_CPU_EMU 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pypwt_amd/csrc/dwt2_inv_coarse_kernels.hpp"

using namespace pdwt;

#define EMU_API extern "C" __attribute__((visibility("default")))

static int cdiv(int a, int b) { return (a + b - 1) / b; }

template <int HLEN, int TX, int TY>
static bool fits(int N0r, int N0c) {  // == coarse3_fits of launch_dwt2_inv_coarse.hip
    using P = InvCoarse3Geom<HLEN, TX, TY>;
    const int r[3] = {N0r / 2, N0r / 4, N0r / 8}, c[3] = {N0c / 2, N0c / 4, N0c / 8};
    const int R[3] = {P::R1, P::R2, P::R3}, W[3] = {P::W1, P::W2, P::W3}, Y[3] = {P::Y1, P::Y2, P::Y3}, X[3] = {P::X1, P::X2, P::X3};
    for (int k = 0; k < 3; k++)
        if (r[k] < R[k] || r[k] < -Y[k] || c[k] < W[k] || c[k] < -X[k]) return false;
    return true;
}

template <int HLEN, int TX, int TY, int NT>
static int run(InvCoarse3Args a, int batch) {
    if (!fits<HLEN, TX, TY>(a.N0r, a.N0c)) return 1;  // declined
    std::vector<float> smem(InvCoarse3Geom<HLEN, TX, TY>::LDS_FLOATS, NAN);
    a.tiles_x = cdiv(a.N0c, 2 * TX);
    a.tiles_y = cdiv(a.N0r, 2 * TY);
    for (int bz = 0; bz < batch; bz++)
        for (int by = 0; by < a.tiles_y; by++)
            for (int bx = 0; bx < a.tiles_x; bx++) {
                std::fill(smem.begin(), smem.end(), NAN);
                dwt2_inv_coarse3_tile<HLEN, TX, TY, NT>(a, bx, by, bz, smem.data());
            }
    return 0;
}

// l1 = H1,V1,D1 [3][batch][N0r/2][N0c/2]; l2 = H2,V2,D2 [3][batch][N0r/4][N0c/4]; l3 = A3,H3,V3,D3 [4][batch][N0r/8][N0c/8]
// shape: 0 = 64x32/512, 1 = 128x16/512, 2 = 64x16/512, 3 = 128x8/256, 4 = 16x4/64.  Returns 0, 1 = the shape does not fit
// these planes (nothing written), negative = bad arguments.
EMU_API int emu_dwt2_inv_coarse3(const float* l1, const float* l2, const float* l3, int batch, int N0r, int N0c, const float* lo,
                                 const float* hi, int hlen, int shape, float* out) {
    if ((hlen & 1) || hlen < 2 || hlen > 8 || (N0r % 8) || (N0c % 32) || N0r < 8 || N0c < 32) return -2;
    InvCoarse3Args a;
    std::memset(&a, 0, sizeof(a));
    a.N0r = N0r; a.N0c = N0c;
    a.out_bstride = (long long)N0r * N0c;
    a.l1_bstride = (long long)(N0r / 2) * (N0c / 2);
    a.l2_bstride = (long long)(N0r / 4) * (N0c / 4);
    a.l3_bstride = (long long)(N0r / 8) * (N0c / 8);
    a.H1 = l1; a.V1 = l1 + batch * a.l1_bstride; a.D1 = l1 + 2 * batch * a.l1_bstride;
    a.H2 = l2; a.V2 = l2 + batch * a.l2_bstride; a.D2 = l2 + 2 * batch * a.l2_bstride;
    a.A3 = l3; a.H3 = l3 + batch * a.l3_bstride; a.V3 = l3 + 2 * batch * a.l3_bstride; a.D3 = l3 + 3 * batch * a.l3_bstride;
    a.out = out;
    for (int i = 0; i < hlen; i++) { a.fb.t[i].x = lo[i]; a.fb.t[i].y = hi[i]; }
    switch (hlen) {
#define X(h)                                                     \
    case h:                                                      \
        switch (shape) {                                         \
            case 0: return run<h, 64, 32, 512>(a, batch);        \
            case 1: return run<h, 128, 16, 512>(a, batch);       \
            case 2: return run<h, 64, 16, 512>(a, batch);        \
            case 3: return run<h, 128, 8, 256>(a, batch);        \
            case 4: return run<h, 16, 4, 64>(a, batch);          \
        }                                                        \
        return -3;
        X(2) X(4) X(6) X(8)
#undef X
    }
    return -2;
}

#ifdef EMU_INV_COARSE_MAIN
// one periodic synthesis level, written out plainly (columns, then rows): a,h,v,d (nr x nc) -> out (2 nr x 2 nc)
static void synth_level(const std::vector<float>& A, const float* H, const float* V, const float* D, int nr, int nc, const float* lo,
                        const float* hi, int hlen, std::vector<float>& out) {
    const int H2 = hlen / 2, C = H2 / 2, S = (H2 & 1) ? 0 : 1;
    std::vector<double> t1((size_t)2 * nr * nc), t2((size_t)2 * nr * nc);
    for (int y = 0; y < 2 * nr; y++)
        for (int x = 0; x < nc; x++) {
            const int p = y + S, par = 1 - (p & 1);
            double s1 = 0, s2 = 0;
            for (int j = 0; j < H2; j++) {
                int k = (p >> 1) - C + j;
                k = ((k % nr) + nr) % nr;
                const int t = hlen - 1 - (2 * j + par);
                s1 += (double)A[(size_t)k * nc + x] * lo[t] + (double)H[(size_t)k * nc + x] * hi[t];
                s2 += (double)V[(size_t)k * nc + x] * lo[t] + (double)D[(size_t)k * nc + x] * hi[t];
            }
            t1[(size_t)y * nc + x] = s1;
            t2[(size_t)y * nc + x] = s2;
        }
    out.assign((size_t)4 * nr * nc, 0.f);
    for (int y = 0; y < 2 * nr; y++)
        for (int x = 0; x < 2 * nc; x++) {
            const int p = x + S, par = 1 - (p & 1);
            double s = 0;
            for (int j = 0; j < H2; j++) {
                int k = (p >> 1) - C + j;
                k = ((k % nc) + nc) % nc;
                const int t = hlen - 1 - (2 * j + par);
                s += t1[(size_t)y * nc + k] * lo[t] + t2[(size_t)y * nc + k] * hi[t];
            }
            out[(size_t)y * 2 * nc + x] = (float)s;
        }
}

int main() {
    unsigned seed = 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)((seed >> 8) & 0xffff) / 32768.f - 1.f; };
    const int sizes[][2] = {{512, 512}, {264, 320}, {72, 288}, {64, 96}, {256, 32}, {32, 256}, {136, 544}, {32, 32}};
    int ran = 0, declined = 0, bad = 0;
    for (int hlen = 2; hlen <= 8; hlen += 2) {
        float lo[8], hi[8];
        for (int i = 0; i < hlen; i++) { lo[i] = 0.5f * rnd(); hi[i] = 0.5f * rnd(); }
        for (const auto& sz : sizes) {
            const int batch = sz[0] == 72 ? 3 : 1;
            const int N0r = sz[0], N0c = sz[1];
            const size_t n1 = (size_t)(N0r / 2) * (N0c / 2), n2 = n1 / 4, n3 = n2 / 4;
            std::vector<float> l1(3 * batch * n1), l2(3 * batch * n2), l3(4 * batch * n3);
            for (float& v : l1) v = rnd();
            for (float& v : l2) v = rnd();
            for (float& v : l3) v = rnd();
            std::vector<float> want((size_t)batch * N0r * N0c);
            for (int b = 0; b < batch; b++) {
                std::vector<float> a3(l3.begin() + b * n3, l3.begin() + (b + 1) * n3), a2, a1, a0;
                synth_level(a3, &l3[(1 * batch + b) * n3], &l3[(2 * batch + b) * n3], &l3[(3 * batch + b) * n3], N0r / 8, N0c / 8, lo, hi, hlen, a2);
                synth_level(a2, &l2[(0 * batch + b) * n2], &l2[(1 * batch + b) * n2], &l2[(2 * batch + b) * n2], N0r / 4, N0c / 4, lo, hi, hlen, a1);
                synth_level(a1, &l1[(0 * batch + b) * n1], &l1[(1 * batch + b) * n1], &l1[(2 * batch + b) * n1], N0r / 2, N0c / 2, lo, hi, hlen, a0);
                std::copy(a0.begin(), a0.end(), want.begin() + (size_t)b * N0r * N0c);
            }
            for (int shape = 0; shape < 5; shape++) {
                std::vector<float> out((size_t)batch * N0r * N0c, NAN);
                const int rc = emu_dwt2_inv_coarse3(l1.data(), l2.data(), l3.data(), batch, N0r, N0c, lo, hi, hlen, shape, out.data());
                if (rc == 1) { declined++; continue; }
                if (rc != 0) { printf("FAIL rc=%d hlen=%d %dx%d shape=%d\n", rc, hlen, N0r, N0c, shape); bad++; continue; }
                ran++;
                double err = 0;
                for (size_t i = 0; i < out.size(); i++) {
                    const double d = std::fabs((double)out[i] - want[i]);
                    if (!(d <= err)) err = d;  // (a NaN makes err NaN)
                }
                // |taps| < 0.5, |coefficients| < 1: three levels of at most 8 x 8 products each stay below ~4^3; fp32 rounding of
                // 3 x 2 x 8 accumulated terms: a few 1e-6 absolute
                if (!(err <= 2e-5)) { printf("FAIL err=%g hlen=%d %dx%d shape=%d\n", err, hlen, N0r, N0c, shape); bad++; }
            }
        }
    }
    printf("emu_inv_coarse: %d runs, %d declined, %d failures\n", ran, declined, bad);
    return bad ? 1 : 0;
}
#endif
