// launch_dwt2_inv_coarse.hip -- launcher of the three-coarse-levels-per-launch inverse for large planes
// (dwt2_inv_coarse_kernels.hpp).  fp32 libraries only (packed-fp32 LDS tiles), even filters of at most 8 taps.
//
// Tile shape: the launch is a latency chain of seven barrier-separated phases behind one load round trip, so the whole
// output should be ONE round of resident workgroups.  The candidates are tried in the order below; the first whose staged
// regions fit the planes and whose resident slots (occupancy query, resident_slots) hold the whole grid is taken, else
// the first that fits.  On the 2048^2 plane of the headline plan (db4): 64 x 32 / 512 -- 79.5 KiB of LDS, two workgroups
// per CU, 512 tiles -- is the one shape that is a single round; 128 x 16 / 512 (84.8 KiB, one per CU) is two rounds,
// 64 x 16 / 512 and 128 x 8 / 256 have 1024 tiles for 768 / 512 slots.  Measured there against the 14.6 us of the two launches it
// replaces (profiles/r07_inv_coarse3_ab.txt): 11.4 / 13.1 / 12.2 / 14.1 us in that order.  The 16 x 4 / 64 shape exists for planes too small
// for the others (the parity tests; the dispatch never sends such planes here).  PDWT_INV_COARSE3_TILE = 1..5 (measurement
// library) forces a shape that fits.
#include "dwt2_inv_coarse_kernels.hpp"

#include <cstdlib>

#include "launch.hpp"
#include "launch_util.hpp"

namespace pdwt {

static std::atomic<int>& coarse3_mode() {
    static std::atomic<int> v{lab_env("PDWT_INV_COARSE3") ? atoi(lab_env("PDWT_INV_COARSE3")) : 1};
    return v;
}
int inv_coarse3_mode() { return coarse3_mode().load(std::memory_order_relaxed); }
int set_inv_coarse3_mode(int v) { return coarse3_mode().exchange(v < 0 ? 0 : (v > 2 ? 2 : v)); }

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int HLEN, int TX, int TY>
static constexpr bool coarse3_fits(int N0r, int N0c) {
    using P = InvCoarse3Geom<HLEN, TX, TY>;
    const int r[3] = {N0r / 2, N0r / 4, N0r / 8}, c[3] = {N0c / 2, N0c / 4, N0c / 8};
    const int R[3] = {P::R1, P::R2, P::R3}, W[3] = {P::W1, P::W2, P::W3}, Y[3] = {P::Y1, P::Y2, P::Y3}, X[3] = {P::X1, P::X2, P::X3};
    for (int k = 0; k < 3; k++)  // one add / sub wraps every staged index: the plane holds the region and its negative origin
        if (r[k] < R[k] || r[k] < -Y[k] || c[k] < W[k] || c[k] < -X[k]) return false;
    return true;
}

template <int HLEN, int TX, int TY, int NT>
static hipError_t coarse3_allow_lds() {
    constexpr size_t lds = (size_t)InvCoarse3Geom<HLEN, TX, TY>::LDS_FLOATS * sizeof(float);
    static_assert(lds <= 150 * 1024, "fits the LDS");
    static std::atomic<bool> big[64] = {};
    return allow_big_lds(dwt2_inv_coarse3_kernel<HLEN, TX, TY, NT>, lds, big);
}

// resident workgroups on the chip (the query counts the dynamic LDS: the opt-in to more than 64 KiB comes first)
template <int HLEN, int TX, int TY, int NT>
static int coarse3_slots() {
    static std::atomic<int> cache[1] = {};
    if (coarse3_allow_lds<HLEN, TX, TY, NT>() != hipSuccess) return 0;
    return resident_slots(dwt2_inv_coarse3_kernel<HLEN, TX, TY, NT>, NT, (size_t)InvCoarse3Geom<HLEN, TX, TY>::LDS_FLOATS * sizeof(float), cache);
}

template <int HLEN, int TX, int TY, int NT>
static hipError_t coarse3_run(InvCoarse3Args& a, int batch, hipStream_t s) {
    constexpr size_t lds = (size_t)InvCoarse3Geom<HLEN, TX, TY>::LDS_FLOATS * sizeof(float);
    const hipError_t e = coarse3_allow_lds<HLEN, TX, TY, NT>();
    if (e != hipSuccess) return e;
    a.tiles_x = cdiv(a.N0c, 2 * TX);
    a.tiles_y = cdiv(a.N0r, 2 * TY);
    const int chunk = (a.tiles_x * a.tiles_y + 7) / 8;
    hipLaunchKernelGGL((dwt2_inv_coarse3_kernel<HLEN, TX, TY, NT>), dim3(8 * chunk, batch), dim3(NT), lds, s, a);
    return hipGetLastError();
}

struct Coarse3Shape {
    int TX, TY;
    bool (*fits)(int, int);
    int (*slots)();
    hipError_t (*run)(InvCoarse3Args&, int, hipStream_t);
};
constexpr int kCoarse3Shapes = 5;
#define PDWT_C3(TX, TY, NT) {TX, TY, [](int r, int c) { return coarse3_fits<HLEN, TX, TY>(r, c); }, coarse3_slots<HLEN, TX, TY, NT>, coarse3_run<HLEN, TX, TY, NT>}
template <int HLEN>
static const Coarse3Shape* coarse3_shapes() {
    static const Coarse3Shape t[kCoarse3Shapes] = {PDWT_C3(64, 32, 512), PDWT_C3(128, 16, 512), PDWT_C3(64, 16, 512), PDWT_C3(128, 8, 256), PDWT_C3(16, 4, 64)};
    return t;
}
#undef PDWT_C3

static const Coarse3Shape* coarse3_table(int hlen) {
    switch (hlen) {
        case 2: return coarse3_shapes<2>();
        case 4: return coarse3_shapes<4>();
        case 6: return coarse3_shapes<6>();
        case 8: return coarse3_shapes<8>();
    }
    return nullptr;
}

// even filters of at most 8 taps; even sizes at all three levels; rows of whole 16-B groups at all three levels; a tile shape whose
// staged regions fit the planes
bool dwt2_inv_coarse3_supported(int hlen, int N0r, int N0c) {
    const Coarse3Shape* t = coarse3_table(hlen);
    if (!t || N0r < 8 || N0c < 32 || (N0r % 8) || (N0c % 32)) return false;
    for (int k = 0; k < kCoarse3Shapes; k++)
        if (t[k].fits(N0r, N0c)) return true;
    return false;
}

// app = A of level l+2; det[3 k + b] = band b (H, V, D) of level l+k -> out (N0r, N0c).  hipErrorNotSupported: declined, nothing ran.
hipError_t launch_dwt2_inv_coarse3(const float* app, float* const det[9], float* out, int N0r, int N0c, int hlen, const FilterBank& fb,
                                   int batch, hipStream_t s) {
    if (!dwt2_inv_coarse3_supported(hlen, N0r, N0c)) return hipErrorNotSupported;
    if (!al16(app) || !al16(out)) return hipErrorNotSupported;
    for (int k = 0; k < 9; k++)
        if (!al16(det[k])) return hipErrorNotSupported;
    InvCoarse3Args a;
    a.A3 = app; a.H3 = det[6]; a.V3 = det[7]; a.D3 = det[8];
    a.H2 = det[3]; a.V2 = det[4]; a.D2 = det[5];
    a.H1 = det[0]; a.V1 = det[1]; a.D1 = det[2];
    a.out = out; a.N0r = N0r; a.N0c = N0c;
    a.out_bstride = (long long)N0r * N0c;
    a.l1_bstride = (long long)(N0r / 2) * (N0c / 2);
    a.l2_bstride = (long long)(N0r / 4) * (N0c / 4);
    a.l3_bstride = (long long)(N0r / 8) * (N0c / 8);
    for (int i = 0; i < kMaxTaps; i++) {
        a.fb.t[i].x = fb.lo[i];
        a.fb.t[i].y = fb.hi[i];
    }
    a.wt_out = wt_stores_take(out, N0r, N0c, a.out_bstride, batch) ? 1 : 0;
    const Coarse3Shape* t = coarse3_table(hlen);
    static const int forced = lab_env("PDWT_INV_COARSE3_TILE") ? atoi(lab_env("PDWT_INV_COARSE3_TILE")) : 0;
    if (forced >= 1 && forced <= kCoarse3Shapes && t[forced - 1].fits(N0r, N0c)) return t[forced - 1].run(a, batch, s);
    int first = -1;
    for (int k = 0; k < kCoarse3Shapes; k++) {
        if (!t[k].fits(N0r, N0c)) continue;
        if (first < 0) first = k;
        const long long tiles = (long long)cdiv(N0c, 2 * t[k].TX) * cdiv(N0r, 2 * t[k].TY) * batch;
        if (tiles <= t[k].slots()) return t[k].run(a, batch, s);
    }
    return t[first].run(a, batch, s);
}

}  // namespace pdwt
