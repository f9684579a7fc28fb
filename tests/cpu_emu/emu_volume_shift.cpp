// emu_volume_shift.cpp -- the index math of the circular shifts of a volume (pypwt_amd/csrc/volume_shift_kernels.hpp: vol_shift_geom_of,
// vol_shift_grid, vol_shift_piece, vol_shift_next, vol_shift_src_row, vol_shift_col, vol_shift_runs, vol_shift_wave, vol_acc) on the
// host (test-only; built by tests/test_emu_volume_shift.py with g++ -DPDWT_CPU_EMU, once more with -DPDWT_DOUBLE, and as a
// stand-alone program under the sanitizers).
//
// Source and destination are heap blocks of exactly the volume's size (256-B aligned like device buffers, or moved off_in / off_out
// values off that alignment, which takes the groups away).  Every workgroup of the launch is walked wavefront by wavefront and lane
// by lane through vol_shift_wave, the function both kernels walk with, with the launchers' own geometry; the grid may be capped
// below the kernels' 2048 so that small volumes reach the stride over the trips too.
#include "../../pypwt_amd/csrc/volume_shift_kernels.hpp"

#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace pdwt;

namespace {

struct Block {
    void* raw = nullptr;
    real_t* p = nullptr;
    // n values, the first of them `off` values behind a 256-B boundary; the block ends with the last value
    Block(long long n, int off) {
        if (posix_memalign(&raw, 256, (size_t)(n + off) * sizeof(real_t))) abort();
        p = static_cast<real_t*>(raw) + off;
    }
    ~Block() { free(raw); }
    Block(const Block&) = delete;
};

struct Walk {
    VolShiftGeom g;
    long long n = 0, bad = 0;
    const real_t* in = nullptr;
    real_t* out = nullptr;
    std::vector<int> written;

    bool in_ok(long long i, int width) {
        if (i < 0 || i + width > n) return false;
        return width == 1 || reinterpret_cast<uintptr_t>(in + i) % (4 * sizeof(real_t)) == 0;
    }
    bool out_ok(long long i, int width) {
        if (i < 0 || i + width > n) return false;
        return width == 1 || reinterpret_cast<uintptr_t>(out + i) % (4 * sizeof(real_t)) == 0;
    }

    // every workgroup of the launch; store1 / store4 do the kernel's arithmetic
    template <typename S1, typename S4>
    void run(int max_grid, S1 store1, S4 store4) {
        written.assign((size_t)n, 0);
        const int grid = vol_shift_grid(g, max_grid);
        if (grid < 1 || grid > max_grid) bad++;
        const real4_t zero4 = {real_t(0), real_t(0), real_t(0), real_t(0)};
        auto ld1 = [&](long long i) {
            if (!in_ok(i, 1)) return bad++, real_t(0);
            return in[i];
        };
        auto ld4 = [&](long long i) {
            if (!in_ok(i, 4)) return bad++, zero4;
            return *reinterpret_cast<const real4_t*>(in + i);
        };
        auto st1 = [&](long long i, real_t x) {
            if (!out_ok(i, 1)) return (void)bad++;
            written[(size_t)i]++;
            store1(i, x);
        };
        auto st4 = [&](long long i, const real4_t& x) {
            if (!out_ok(i, 4)) return (void)bad++;
            for (int j = 0; j < 4; j++) written[(size_t)(i + j)]++;
            store4(i, x);
        };
        const long long waves = (long long)grid * kVolShiftWaves;
        for (int blk = 0; blk < grid; blk++)
            for (int tid = 0; tid < kVolShiftThreads; tid++)
                for (long long trip = (long long)blk * kVolShiftWaves + (tid >> 6); trip < g.trips; trip += waves) {
                    const int lane = tid & 63;
                    if (g.mode == 2) vol_shift_wave<2>(g, trip, lane, ld1, ld4, st1, st4);
                    else if (g.mode == 1) vol_shift_wave<1>(g, trip, lane, ld1, ld4, st1, st4);
                    else vol_shift_wave<0>(g, trip, lane, ld1, ld4, st1, st4);
                }
        for (long long i = 0; i < n; i++)
            if (written[(size_t)i] != 1) bad++;
    }

    // the pieces cover the volume in order, counting agrees with dividing, and the two runs of a piece are what the column wrap gives
    void check_pieces() {
        int z = 0, r = 0, seg = 0;
        for (long long piece = 0; piece < g.pieces; piece++) {
            int pz, pr, ps;
            vol_shift_piece(g, piece, &pz, &pr, &ps);
            if (pz != z || pr != r || ps != seg || z >= g.Nz) bad++;
            const int c0 = seg * kVolShiftSeg, c1 = c0 + kVolShiftSeg < g.Nc ? c0 + kVolShiftSeg : g.Nc;
            int m;
            vol_shift_runs(g, c0, c1, &m);
            if (m < c0 || m > c1) bad++;
            for (int c = c0; c < c1; c++)
                if (vol_shift_col(g, c) != (c < m ? c + g.Nc - g.sc : c - g.sc)) bad++;
            vol_shift_next(g, &z, &r, &seg);
        }
        if (z != g.Nz || r != 0 || seg != 0) bad++;
    }
};

}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

// vol_circshift_kernel: out (n values; the caller prefills it, with NaN) = circshift(in, sz, sr, sc), the shifts as a caller gives
// them.  info = {mode, workgroups, pieces, trips, reduced sz, sr, sc}.  Returns the number of faults: an access outside the volume, a
// group off its alignment, an output value not written exactly once, a piece that counting and dividing place differently.
EMU_API long long emu_vs_shift(int Nz, int Nr, int Nc, long long sz, long long sr, long long sc, int max_grid, int off_in, int off_out,
                               const real_t* in, real_t* out, long long* info) {
    const long long n = (long long)Nz * Nr * Nc;
    Block a(n, off_in), b(n, off_out);
    memcpy(a.p, in, (size_t)n * sizeof(real_t));
    memcpy(b.p, out, (size_t)n * sizeof(real_t));
    Walk w;
    w.g = vol_shift_geom_of(Nz, Nr, Nc, sz, sr, sc, false, a.p, b.p);
    w.n = n, w.in = a.p, w.out = b.p;
    w.check_pieces();
    w.run(
        max_grid, [&](long long i, real_t x) { b.p[i] = x; }, [&](long long i, const real4_t& x) { *reinterpret_cast<real4_t*>(b.p + i) = x; });
    memcpy(out, b.p, (size_t)n * sizeof(real_t));
    if (info) {
        info[0] = w.g.mode, info[1] = vol_shift_grid(w.g, max_grid), info[2] = w.g.pieces, info[3] = w.g.trips;
        info[4] = w.g.sz, info[5] = w.g.sr, info[6] = w.g.sc;
    }
    return w.bad;
}

// vol_unshift_acc_kernel, nshifts launches: acc (n values, prefilled by the caller) = sum_s w circshift(rec_s, -shift_s), the first
// launch with `first`.  rec_s = recs + s * rec_stride.  modes[s] = the mode of launch s.  Returns the number of faults, as above.
EMU_API long long emu_vs_acc(int Nz, int Nr, int Nc, int nshifts, const long long* shifts, int max_grid, int off_in, int off_out,
                             const real_t* recs, long long rec_stride, real_t wgt, real_t* acc, long long* modes) {
    const long long n = (long long)Nz * Nr * Nc;
    Block a(n, off_in), b(n, off_out);
    memcpy(b.p, acc, (size_t)n * sizeof(real_t));
    long long bad = 0;
    for (int s = 0; s < nshifts; s++) {
        memcpy(a.p, recs + s * rec_stride, (size_t)n * sizeof(real_t));
        Walk w;
        w.g = vol_shift_geom_of(Nz, Nr, Nc, shifts[3 * s], shifts[3 * s + 1], shifts[3 * s + 2], true, a.p, b.p);
        w.n = n, w.in = a.p, w.out = b.p;
        const int first = s == 0;
        w.run(
            max_grid, [&](long long i, real_t x) { b.p[i] = vol_acc(first ? real_t(0) : b.p[i], wgt, x, first); },
            [&](long long i, const real4_t& x) {
                const real_t v[4] = {x.x, x.y, x.z, x.w};
                for (int j = 0; j < 4; j++) b.p[i + j] = vol_acc(first ? real_t(0) : b.p[i + j], wgt, v[j], first);
            });
        if (modes) modes[s] = w.g.mode;
        bad += w.bad;
    }
    memcpy(acc, b.p, (size_t)n * sizeof(real_t));
    return bad;
}

#ifdef EMU_VOLUME_SHIFT_MAIN
// Stand-alone form for the sanitizer run: reads records {int64 Nz, Nr, Nc, sz, sr, sc, max_grid, off_in, off_out; Nz Nr Nc values}
// from the file named first; writes, per record, the shifted volume and then the mean of three unshifts -- of the record's own
// shift s, of s + (1, 2, 3) and of (-5, 0, 7) - s, all of the record's values, weight 1/3 -- to the file named second; prints
// "shift-faults acc-faults" per record.
#include <math.h>
#include <stdio.h>
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!f || !out) return 2;
    long long head[9];
    while (fread(head, sizeof(long long), 9, f) == 9) {
        const int Nz = (int)head[0], Nr = (int)head[1], Nc = (int)head[2];
        const size_t n = (size_t)Nz * Nr * Nc;
        std::vector<real_t> x(n), y(n, (real_t)NAN), acc(n, (real_t)NAN);
        if (fread(x.data(), sizeof(real_t), n, f) != n) return 3;
        const long long bad_shift =
            emu_vs_shift(Nz, Nr, Nc, head[3], head[4], head[5], (int)head[6], (int)head[7], (int)head[8], x.data(), y.data(), nullptr);
        const long long sh[9] = {head[3], head[4], head[5], head[3] + 1, head[4] + 2, head[5] + 3, -5 - head[3], -head[4], 7 - head[5]};
        const long long bad_acc = emu_vs_acc(Nz, Nr, Nc, 3, sh, (int)head[6], (int)head[7], (int)head[8], x.data(), 0,
                                             (real_t)(1.0 / 3.0), acc.data(), nullptr);
        printf("%lld %lld\n", bad_shift, bad_acc);
        if (fwrite(y.data(), sizeof(real_t), n, out) != n || fwrite(acc.data(), sizeof(real_t), n, out) != n) return 3;
    }
    fclose(f);
    fclose(out);
    return 0;
}
#endif
