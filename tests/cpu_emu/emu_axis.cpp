// emu_axis.cpp -- the depth-axis kernels of a volume (pypwt_amd/csrc/dwt3_axis_kernels.hpp) on the host: the tile functions
// are compiled with g++ -DPDWT_CPU_EMU and run workgroup by workgroup over the launchers' grid.  Built by
// tests/test_emu_axis.py as a shared library (fp32 and -DPDWT_DOUBLE) and, with -DEMU_AXIS_MAIN, as a stand-alone program
// for the address and undefined-behaviour sanitizers: there every buffer is a heap block of exactly the input's / output's size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pypwt_amd/csrc/dwt3_axis_kernels.hpp"

using namespace pdwt;

namespace {

constexpr int NT = kDwt3NT;

template <int HLEN, int VEC>
void run(const Dwt3Args& a, bool inverse) {
    const long long gx = dwt3_col_groups(a.P, VEC);
    const int steps = inverse ? dwt3_inv_steps(a.Nz, HLEN) : dwt3_fwd_steps(a.Nz);
    const int gy = (steps + a.seg - 1) / a.seg;
    for (int by = 0; by < gy; by++)
        for (long long bx = 0; bx < gx; bx++) {
            if (inverse) dwt3_depth_inv_tile<HLEN, VEC, NT>(a, a.fb.lo, a.fb.hi, bx, by);
            else dwt3_depth_fwd_tile<HLEN, VEC, NT>(a, a.fb.lo, a.fb.hi, bx, by);
        }
}

template <int HLEN>
int run_width(const Dwt3Args& a, int width, bool inverse) {
    constexpr int W = dwt3_wide(HLEN);
    if (width == 1) {
        run<HLEN, 1>(a, inverse);
        return 0;
    }
    if constexpr (W > 1) {
        if (width == W && a.P % W == 0) {
            run<HLEN, W>(a, inverse);
            return 0;
        }
    }
    return -1;
}

}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

// the widest access the launcher would pick for a slice of P samples (buffers aligned)
EMU_API int emu_axis_width(long long P, int hlen) {
    return dwt3_width(nullptr, nullptr, P, hlen);
}

EMU_API int emu_axis_steps(int Nz, int hlen, int inverse) { return inverse ? dwt3_inv_steps(Nz, hlen) : dwt3_fwd_steps(Nz); }

// the host chooser of launch_depth3.hip for `slots` resident workgroups
EMU_API int emu_axis_seg(int Nz, long long P, int hlen, int width, int inverse, int slots) {
    return dwt3_pick_seg(emu_axis_steps(Nz, hlen, inverse), dwt3_col_groups(P, width), hlen, slots);
}

// forward: in [Nz][P] -> out [2 div2(Nz)][P]; inverse: in [2 div2(Nz)][P] -> out [Nz][P].  lo / hi: hlen taps.  0, or -1 for
// a combination that is not built
EMU_API int emu_axis_run(const real_t* in, real_t* out, int Nz, long long P, int hlen, const real_t* lo, const real_t* hi, int seg,
                         int width, int inverse) {
    if (hlen < 1 || hlen > kMaxTaps) return -1;
    Dwt3Args a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.out = out;
    a.Nz = Nz;
    a.Nh = dwt3_div2(Nz);
    a.P = P;
    a.seg = seg;
    for (int i = 0; i < hlen; i++) a.fb.lo[i] = lo[i], a.fb.hi[i] = hi[i];
    switch (hlen) {  // every even length the launchers instantiate: one list (kernels_common.hpp)
#define X(h) case h: return run_width<h>(a, width, inverse != 0);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return -1;
}

#ifdef EMU_AXIS_MAIN
// Stand-alone sanitizer run.  Reads records {int64 Nz, P, hlen, seg, width, inverse; real lo[hlen], hi[hlen]; real in[...]} from
// argv[1], runs each on heap blocks of exactly the input's and the output's size and writes the outputs, back to back, to argv[2].
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    long long h[6];
    int records = 0;
    while (fread(h, sizeof(long long), 6, f) == 6) {
        const int Nz = (int)h[0], hlen = (int)h[2], seg = (int)h[3], width = (int)h[4], inverse = (int)h[5];
        const long long P = h[1];
        const size_t stack = (size_t)2 * dwt3_div2(Nz) * P, vol = (size_t)Nz * P;
        const size_t n_in = inverse ? stack : vol, n_out = inverse ? vol : stack;
        real_t* lo = (real_t*)malloc(sizeof(real_t) * hlen);
        real_t* hi = (real_t*)malloc(sizeof(real_t) * hlen);
        real_t* in = (real_t*)malloc(sizeof(real_t) * n_in);
        real_t* out = (real_t*)malloc(sizeof(real_t) * n_out);
        if (fread(lo, sizeof(real_t), hlen, f) != (size_t)hlen || fread(hi, sizeof(real_t), hlen, f) != (size_t)hlen ||
            fread(in, sizeof(real_t), n_in, f) != n_in)
            return 3;
        memset(out, 0xff, sizeof(real_t) * n_out);
        if (emu_axis_run(in, out, Nz, P, hlen, lo, hi, seg, width, inverse) != 0) return 4;
        if (fwrite(out, sizeof(real_t), n_out, g) != n_out) return 5;
        free(lo), free(hi), free(in), free(out);
        records++;
    }
    fclose(f);
    fclose(g);
    printf("%d\n", records);
    return 0;
}
#endif
