// emu_swt_axis.cpp -- the depth-axis a-trous kernels of a stationary volume (pypwt_amd/csrc/swt3_axis_kernels.hpp) on the host: the
// tile functions are compiled with g++ -DPDWT_CPU_EMU and run workgroup by workgroup over the launchers' grid.  Built by
// tests/test_emu_swt_axis.py as a shared library (fp32 and -DPDWT_DOUBLE) and, with -DEMU_SWT_AXIS_MAIN, as a stand-alone program
// for the address and undefined-behaviour sanitizers: there every buffer is a heap block of exactly the input's / output's size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pypwt_amd/csrc/swt3_axis_kernels.hpp"

using namespace pdwt;

namespace {

constexpr int NT = kSwt3NT;

template <int HLEN, int VEC>
void run(const Swt3Args& a, bool inverse) {
    const long long gx = swt3_col_groups(a.P, VEC);
    const int gy = a.orbits * a.nseg;
    for (int by = 0; by < gy; by++)
        for (long long bx = 0; bx < gx; bx++) {
            if (inverse) swt3_depth_inv_tile<HLEN, VEC, NT>(a, a.fb.lo, a.fb.hi, bx, by);
            else swt3_depth_fwd_tile<HLEN, VEC, NT>(a, a.fb.lo, a.fb.hi, bx, by);
        }
}

template <int HLEN, bool INV>
int run_width(const Swt3Args& a, int width) {
    constexpr int W = swt3_wide(HLEN, INV);
    if (width == 1) {
        run<HLEN, 1>(a, INV);
        return 0;
    }
    if constexpr (W > 1) {
        if (width == W && a.P % W == 0) {
            run<HLEN, W>(a, INV);
            return 0;
        }
    }
    return -1;
}

}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

// the widest access the launcher would pick for a slice of P samples (buffers aligned)
EMU_API int emu_swt_axis_width(long long P, int hlen, int inverse) { return swt3_width(nullptr, nullptr, P, hlen, inverse != 0); }

EMU_API int emu_swt_axis_orbits(int Nz, int f) { return swt3_orbits(f, Nz); }

EMU_API int emu_swt_axis_steps(int Nz, int f) { return swt3_steps(f, Nz); }

// the host chooser of launch_depth3.hip for `slots` resident workgroups
EMU_API int emu_swt_axis_seg(int Nz, int f, long long P, int hlen, int width, int slots) {
    return swt3_pick_seg(swt3_steps(f, Nz), swt3_col_groups(P, width), swt3_orbits(f, Nz), hlen, slots);
}

// the output slices the launch geometry visits for `seg` steps per segment, in grid order: visited[0 .. return value); the
// test checks that they are 0 .. Nz - 1, each once
EMU_API int emu_swt_axis_cover(int Nz, int f, int seg, int* visited, int capacity) {
    Swt3Args a;
    memset(&a, 0, sizeof(a));
    swt3_geometry(a, Nz, f, seg);
    int n = 0;
    for (int by = 0; by < a.orbits * a.nseg; by++) {
        const int o = by / a.nseg, t0 = (by - o * a.nseg) * a.seg;
        const int t1 = t0 + a.seg < a.steps ? t0 + a.seg : a.steps;
        int g = swt3_out_slice(o, t0, a.fm, a.Nz);
        for (int t = t0; t < t1; t++) {
            if (n < capacity) visited[n] = g;
            n++;
            g = swt3_next(g, a.fm, a.Nz);
        }
    }
    return n;
}

// forward: in [Nz][P] -> out [2 Nz][P]; inverse: in [2 Nz][P] -> out [Nz][P].  lo / hi: hlen taps.  0, or -1 for a combination
// that is not built
EMU_API int emu_swt_axis_run(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const real_t* lo, const real_t* hi,
                             int seg, int width, int inverse) {
    if (hlen < 1 || hlen > kMaxTaps || Nz < 1 || f < 1 || P < 1 || seg < 1) return -1;
    Swt3Args a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.out = out;
    a.P = P;
    swt3_geometry(a, Nz, f, seg);
    for (int i = 0; i < hlen; i++) a.fb.lo[i] = lo[i], a.fb.hi[i] = hi[i];
    switch (hlen) {  // every even length the launchers instantiate: one list (kernels_common.hpp)
#define X(h) case h: return inverse ? run_width<h, true>(a, width) : run_width<h, false>(a, width);
        PDWT_EVEN_HLENS(X)
#undef X
    }
    return -1;
}

#ifdef EMU_SWT_AXIS_MAIN
// Stand-alone sanitizer run.  Reads records {int64 Nz, P, f, hlen, seg, width, inverse; real lo[hlen], hi[hlen]; real in[...]} from
// argv[1], runs each on heap blocks of exactly the input's and the output's size and writes the outputs, back to back, to argv[2].
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    long long h[7];
    int records = 0;
    while (fread(h, sizeof(long long), 7, f) == 7) {
        const int Nz = (int)h[0], dil = (int)h[2], hlen = (int)h[3], seg = (int)h[4], width = (int)h[5], inverse = (int)h[6];
        const long long P = h[1];
        const size_t stack = (size_t)2 * Nz * P, vol = (size_t)Nz * P;
        const size_t n_in = inverse ? stack : vol, n_out = inverse ? vol : stack;
        real_t* lo = (real_t*)malloc(sizeof(real_t) * hlen);
        real_t* hi = (real_t*)malloc(sizeof(real_t) * hlen);
        real_t* in = (real_t*)malloc(sizeof(real_t) * n_in);
        real_t* out = (real_t*)malloc(sizeof(real_t) * n_out);
        if (fread(lo, sizeof(real_t), hlen, f) != (size_t)hlen || fread(hi, sizeof(real_t), hlen, f) != (size_t)hlen ||
            fread(in, sizeof(real_t), n_in, f) != n_in)
            return 3;
        memset(out, 0xff, sizeof(real_t) * n_out);
        if (emu_swt_axis_run(in, out, Nz, P, dil, hlen, lo, hi, seg, width, inverse) != 0) return 4;
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
