// emu_volume_ops.cpp -- the index math of pypwt_amd/csrc/volume_ops_kernels.hpp (the range table of a volume's K-term operators,
// the piece -> range map, the (level, band, slice) -> sub-band map) on the host (test-only; built by tests/test_emu_volume_ops.py
// with g++ -DPDWT_CPU_EMU, once more with -DPDWT_DOUBLE, and as a stand-alone program under the sanitizers).
//
// The per-level arenas are laid out as a one-level batched 2D plan lays out its coefficient region (plan.cpp: bands A, H, V, D of
// [2 div2(Nz)][rows][cols], each padded to 64 values) in heap blocks of exactly that size.  Every sub-band is filled with its
// `num`, or with the caller's values; the intermediates (the depth-low half of band A below the last level) and the padding hold
// a huge sentinel.  A workgroup is walked as sweep_range walks it: single values up to the first whole group of four (counted
// from the arena's base), whole groups, single values behind the last one.
#include "../../pypwt_amd/csrc/volume_ops_kernels.hpp"

#include <stdlib.h>

#include <vector>

using namespace pdwt;

namespace {

int div2(int n) { return (n + (n & 1)) / 2; }
long long pad64(long long n) { return (n + 63) & ~63LL; }

const real_t kSentinel = sizeof(real_t) == 4 ? (real_t)3.0e38 : (real_t)1.0e300;

struct Volume {
    int L = 0;
    std::vector<int> nz, nr, nc;           // [l]: sizes of A_l
    std::vector<real_t*> arena;            // [l - 1]
    std::vector<long long> elems;          // [l - 1]: values of the coefficient region
    std::vector<std::vector<char>> seen;   // [l - 1][index]: visits
    VolRangeTable t{};
    long long total = 0;

    Volume(int Nz, int Nr, int Nc, int levels, int which) : L(levels), nz(1, Nz), nr(1, Nr), nc(1, Nc) {
        t.nranges = 0;
        for (int l = 1; l <= L; l++) {
            nz.push_back(div2(nz[l - 1])), nr.push_back(div2(nr[l - 1])), nc.push_back(div2(nc[l - 1]));
            const long long band = pad64(2LL * nz[l] * nr[l] * nc[l]);
            const long long off[4] = {0, band, 2 * band, 3 * band};
            elems.push_back(4 * band);
            real_t* a = static_cast<real_t*>(aligned_alloc(256, (size_t)(4 * band) * sizeof(real_t)));
            for (long long i = 0; i < 4 * band; i++) a[i] = kSentinel;
            arena.push_back(a);
            seen.emplace_back((size_t)(4 * band), 0);
            vol_ranges_add_level(t, a, off, nz[l], (long long)nr[l] * nc[l]);
        }
        total = vol_ranges_finish(t, arena[L - 1], 0, nz[L], (long long)nr[L] * nc[L], which ? 2048 : 1024, which ? 4096 : 8192);
    }
    ~Volume() {
        for (real_t* a : arena) free(a);
    }
    int nbands() const { return 1 + 7 * L; }
    long long count(int num) const {
        int level, half, band;
        vol_locate(num, L, &level, &half, &band);
        return (long long)nz[level] * nr[level] * nc[level];
    }
    real_t* sub(int num) const {
        int level, half, band;
        vol_locate(num, L, &level, &half, &band);
        const long long n = count(num);
        return arena[level - 1] + band * pad64(2 * n) + half * n;
    }
    int level_of(const real_t* base) const {
        for (int l = 1; l <= L; l++)
            if (arena[l - 1] == base) return l;
        return 0;
    }
    int blocks(int do_app) const { return t.blk[do_app ? t.nranges : t.nranges - 1]; }

    // workgroup `blk` as sweep_range walks it: f(level, index) for every value; returns the number of groups of four that are
    // not 16-B (fp64: 32-B) aligned or leave the piece -- 0 for a sound table
    template <typename F>
    long long walk(int blk, F f) const {
        long long a, e, bad = 0;
        const int r = vol_piece(t, blk, &a, &e);
        const real_t* base = t.base[r];
        const int level = level_of(base);
        if (!level || a < t.first[r] || e > t.end[r] || a >= e || e > elems[level - 1]) return 1 + (e > a ? e - a : 0);
        long long a4 = (a + 3) & ~3LL, e4 = e & ~3LL;
        if (a4 > e) a4 = e;
        if (e4 < a4) e4 = a4;
        for (long long i = a; i < a4; i++) f(level, i);
        for (long long i = e4; i < e; i++) f(level, i);
        for (long long g = a4 / 4; g < e4 / 4; g++) {
            if (reinterpret_cast<uintptr_t>(base + 4 * g) % (4 * sizeof(real_t))) bad++;
            for (int j = 0; j < 4; j++) f(level, 4 * g + j);
        }
        return bad;
    }
};

}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API int emu_vol_num_of(int level, int nlevels, int band, int img, int half) { return vol_num_of(level, nlevels, band, img, half); }

EMU_API void emu_vol_locate(int num, int nlevels, int* level, int* half, int* band) { vol_locate(num, nlevels, level, half, band); }

// Every workgroup of the table (which: 0 the histogram passes', 1 the keep sweep's) over arenas whose sub-bands hold their `num`:
// counts[num] = visits of values equal to num; info = {ranges, chunk, workgroups, swept elements of the table}.  Returns the number
// of faults: a sentinel, a second visit, a piece outside its range, a misaligned group.
EMU_API long long emu_vol_walk(int Nz, int Nr, int Nc, int L, int do_app, int which, long long* counts, long long* info) {
    Volume v(Nz, Nr, Nc, L, which);
    for (int num = 0; num < v.nbands(); num++) {
        real_t* p = v.sub(num);
        for (long long i = 0; i < v.count(num); i++) p[i] = (real_t)num;
        counts[num] = 0;
    }
    long long bad = 0, wrong = 0;
    for (int blk = 0; blk < v.blocks(do_app); blk++)
        bad += v.walk(blk, [&](int level, long long i) {
            const real_t x = v.arena[level - 1][i];
            if (x == kSentinel || v.seen[level - 1][i]++) wrong++;
            else counts[(int)x]++;
        });
    info[0] = v.t.nranges, info[1] = v.t.chunk, info[2] = v.blocks(do_app), info[3] = v.total;
    return bad + wrong;
}

// select_magnitude + keep_largest over the range tables on the caller's values (`flat`: the sub-bands one behind the other in
// `num` order, overwritten with what the keep sweep leaves).  Returns the histogram sweeps that ran, or -1 - faults when a
// sentinel was read or changed.
EMU_API int emu_vol_keep_largest(int Nz, int Nr, int Nc, int L, int do_app, long long k, real_t* flat, real_t* threshold,
                                 unsigned long long* kept) {
    Volume hist(Nz, Nr, Nc, L, 0), keep(Nz, Nr, Nc, L, 1);
    long long at = 0;
    for (int num = 0; num < hist.nbands(); num++) {
        for (long long i = 0; i < hist.count(num); i++) hist.sub(num)[i] = keep.sub(num)[i] = flat[at + i];
        at += hist.count(num);
    }
    unsigned long long n = 0;
    for (int num = do_app ? 0 : 1; num < hist.nbands(); num++) n += (unsigned long long)hist.count(num);
    long long faults = 0;
    SelectState st = {};
    std::vector<unsigned> h(kSelectMaxBins), part(256), part16(16);
    int sweeps = 0;
    for (int pass = 0; pass < kSelectPasses; pass++) {  // vol_select_hist_kernel, select_walk_rank_kernel
        const int bits = select_pass_bits(pass), shift = select_pass_shift(pass), bins = 1 << bits;
        for (int b = 0; b < kSelectMaxBins; b++) h[b] = 0;
        const bool skip = pass == 0 ? select_rank_flag(k, n) != 0 : st.empty != 0;
        if (!skip) {
            sweeps++;
            unsigned unused = kSelectNoDigit;
            for (int blk = 0; blk < hist.blocks(do_app); blk++)
                faults += hist.walk(blk, [&](int level, long long i) {
                    const int d = select_classify(select_key(hist.arena[level - 1][i]), shift, bits, (select_key_t)st.lo_prefix, 0, 0, &unused);
                    if (d >= 0) h[d]++;
                });
        }
        for (int t = 0; t < 256; t++) part[t] = select_part_sum(h.data(), bins, t);
        for (int g = 0; g < 16; g++) part16[g] = select_part16_sum(part.data(), g);
        select_rank_step(st, pass, h.data(), part.data(), part16.data(), k, n);
    }
    const select_key_t key = select_rank_result(st, k, n, kept);
    *threshold = select_rank_value(key);
    const select_key_t mag = ~(select_key_t)0 >> 1;
    if (key != 0)  // vol_keep_kernel: a key of 0 returns before it reads
        for (int blk = 0; blk < keep.blocks(do_app); blk++)
            faults += keep.walk(blk, [&](int level, long long i) {
                real_t& x = keep.arena[level - 1][i];
                x = key > mag ? real_t(0) : vol_keep(x, key);
            });
    // what is not a sub-band must still be the sentinel
    for (int l = 1; l <= L; l++) {
        std::vector<char> own((size_t)keep.elems[l - 1], 0);
        for (int num = 0; num < keep.nbands(); num++) {
            int level, half, band;
            vol_locate(num, L, &level, &half, &band);
            if (level == l)
                for (long long i = 0; i < keep.count(num); i++) own[(size_t)(keep.sub(num) - keep.arena[l - 1] + i)] = 1;
        }
        for (long long i = 0; i < keep.elems[l - 1]; i++)
            if (!own[(size_t)i] && keep.arena[l - 1][i] != kSentinel) faults++;
    }
    at = 0;
    for (int num = 0; num < keep.nbands(); num++) {
        for (long long i = 0; i < keep.count(num); i++) flat[at + i] = keep.sub(num)[i];
        at += keep.count(num);
    }
    return faults ? (int)(-1 - faults) : sweeps;
}

#ifdef EMU_VOLUME_OPS_MAIN
// Stand-alone form for the sanitizer run: reads records {int64 Nz, Nr, Nc, L, do_app, k, n, n values} from the file named first and
// writes the swept values behind each other to the file named second; prints "walk-faults-hist walk-faults-keep status
// threshold-as-hex-bits kept" per record.
#include <stdio.h>
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!f || !out) return 2;
    long long head[7];
    while (fread(head, sizeof(long long), 7, f) == 7) {
        std::vector<real_t> x((size_t)head[6]);
        if (head[6] > 0 && fread(x.data(), sizeof(real_t), x.size(), f) != x.size()) return 3;
        const int Nz = (int)head[0], Nr = (int)head[1], Nc = (int)head[2], L = (int)head[3], do_app = (int)head[4];
        std::vector<long long> counts((size_t)(1 + 7 * L));
        long long info[4];
        const long long bad_hist = emu_vol_walk(Nz, Nr, Nc, L, do_app, 0, counts.data(), info);
        const long long bad_keep = emu_vol_walk(Nz, Nr, Nc, L, do_app, 1, counts.data(), info);
        real_t t = 0;
        unsigned long long kept = 0, bits = 0;
        const int status = emu_vol_keep_largest(Nz, Nr, Nc, L, do_app, head[5], x.data(), &t, &kept);
        __builtin_memcpy(&bits, &t, sizeof(t));
        printf("%lld %lld %d %llx %llu\n", bad_hist, bad_keep, status, bits, kept);
        if (fwrite(x.data(), sizeof(real_t), x.size(), out) != x.size()) return 3;
    }
    fclose(f);
    fclose(out);
    return 0;
}
#endif
