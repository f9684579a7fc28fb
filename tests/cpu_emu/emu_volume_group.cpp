// emu_volume_group.cpp -- the index math and the arithmetic of the GROUP operators of a volume (pypwt_amd/csrc/volume_ops_kernels.hpp:
// VolGroupTable, vol_group_piece, vol_group_split, vol_group_sweep, vol_sumsq_add, vol_group_res, vol_group_sq) on the host (test-only; built by
// tests/test_emu_volume_group.py with g++ -DPDWT_CPU_EMU, once more with -DPDWT_DOUBLE, and as a stand-alone program under the
// sanitizers).
//
// The coefficients are laid out as both kinds of volume lay them out, in heap blocks of exactly the coefficient regions' size:
//   decimated   per level the coefficient region of a one-level batched 2D plan: bands A, H, V, D of [2 div2(Nz)][rows][cols], each
//               padded to 64 values (plan.cpp);
//   stationary  one block of 4 L band arrays [2 Nz][Nr Nc], each padded to 256 bytes (volume.cpp: swt_layout).
// Every sub-band holds its `num`, or the caller's values; the intermediates (the depth-low half of band A below the last level)
// and the padding hold a huge sentinel.  Every workgroup of the table is walked by its 256 threads through vol_group_sweep, the
// function the kernels walk with.
#include "../../pypwt_amd/csrc/volume_ops_kernels.hpp"

#include <stdlib.h>

#include <vector>

using namespace pdwt;

namespace {

int div2(int n) { return (n + (n & 1)) / 2; }
long long pad64(long long n) { return (n + 63) & ~63LL; }

const real_t kSentinel = sizeof(real_t) == 4 ? (real_t)3.0e38 : (real_t)1.0e300;

struct Volume {
    int L = 0, swt = 0;
    std::vector<int> nz, nr, nc;       // [l]: sizes of A_l (stationary: the volume's at every level)
    std::vector<real_t*> block;        // the heap blocks: one per level, or one in all
    std::vector<long long> elems;      // values of each block
    std::vector<real_t*> band;         // [4 (l - 1) + b]
    VolGroupTable t{};
    long long total = 0;

    Volume(int Nz, int Nr, int Nc, int levels, int stationary) : L(levels), swt(stationary), nz(1, Nz), nr(1, Nr), nc(1, Nc) {
        for (int l = 1; l <= L; l++) {
            nz.push_back(swt ? Nz : div2(nz[l - 1])), nr.push_back(swt ? Nr : div2(nr[l - 1])), nc.push_back(swt ? Nc : div2(nc[l - 1]));
        }
        if (swt) {
            const long long per = (long long)(((size_t)(2 * count(1)) * sizeof(real_t) + 255) / 256 * 256 / sizeof(real_t));
            real_t* a = alloc(4LL * L * per);
            for (int k = 0; k < 4 * L; k++) band.push_back(a + k * per);
        } else {
            for (int l = 1; l <= L; l++) {
                const long long per = pad64(2 * count(1 + 7 * (l - 1)));
                real_t* a = alloc(4 * per);
                for (int b = 0; b < 4; b++) band.push_back(a + b * per);
            }
        }
        t.nlevels = 0;
        for (int l = 1; l <= L; l++) vol_group_add_level(t, &band[4 * (l - 1)], level_n(l), l == L);
        total = vol_group_finish(t, 2048, 2048);
    }
    ~Volume() {
        for (real_t* a : block) free(a);
    }
    real_t* alloc(long long n) {
        real_t* a = static_cast<real_t*>(aligned_alloc(256, (size_t)n * sizeof(real_t)));
        for (long long i = 0; i < n; i++) a[i] = kSentinel;
        block.push_back(a);
        elems.push_back(n);
        return a;
    }
    int nbands() const { return 1 + 7 * L; }
    long long level_n(int l) const { return (long long)nz[l] * nr[l] * nc[l]; }
    long long count(int num) const {
        int level, half, b;
        vol_locate(num, L, &level, &half, &b);
        return level_n(level);
    }
    real_t* sub(int num) const {
        int level, half, b;
        vol_locate(num, L, &level, &half, &b);
        return band[4 * (level - 1) + b] + half * level_n(level);
    }
    void fill(const real_t* flat) {
        long long at = 0;
        for (int num = 0; num < nbands(); num++) {
            for (long long i = 0; i < count(num); i++) sub(num)[i] = flat ? flat[at + i] : (real_t)num;
            at += count(num);
        }
    }
    void read(real_t* flat) const {
        long long at = 0;
        for (int num = 0; num < nbands(); num++) {
            for (long long i = 0; i < count(num); i++) flat[at + i] = sub(num)[i];
            at += count(num);
        }
    }
    // what is not a sub-band must still be the sentinel
    long long touched() const {
        long long bad = 0;
        for (size_t k = 0; k < block.size(); k++) {
            std::vector<char> own((size_t)elems[k], 0);
            for (int num = 0; num < nbands(); num++) {
                real_t* p = sub(num);
                if (p >= block[k] && p < block[k] + elems[k])
                    for (long long i = 0; i < count(num); i++) own[(size_t)(p - block[k] + i)] = 1;
            }
            for (long long i = 0; i < elems[k]; i++)
                if (!own[(size_t)i] && block[k][i] != kSentinel) bad++;
        }
        return bad;
    }
    int blocks() const { return t.blk[t.nlevels]; }

    // Workgroup `blk`, thread by thread: f(l, i, tid) for every position (l = level index), and g(pointer) for every member of
    // every group of four before its positions are handed to f.  Returns the faults of the geometry: a piece outside its level,
    // a group that leaves the piece or is not 16-B (fp64: 32-B) aligned for one of its members.
    template <typename F>
    long long walk(int blk, int do_app, F f) const {
        long long a, e, bad = 0;
        const int l = vol_group_piece(t, blk, &a, &e);
        if (l < 0 || l >= L || a < 0 || a >= e || e > t.n[l]) return 1;
        const int nm = 7 + ((do_app && t.m[l][7]) ? 1 : 0);
        for (int tid = 0; tid < kVolGroupThreads; tid++)
            vol_group_sweep(
                t.n[l], a, e, tid, kVolGroupThreads, [&](long long i) { f(l, i, tid); },
                [&](long long i) {
                    if (i < a || i + 4 > e) bad++;
                    for (int k = 0; k < nm; k++)
                        if (reinterpret_cast<uintptr_t>(t.m[l][k] + i) % (4 * sizeof(real_t))) bad++;
                    for (int j = 0; j < 4; j++) f(l, i + j, tid);
                });
        return bad;
    }
};

}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

// Every workgroup of the table over sub-bands that hold their `num`: counts[num] = visits of values equal to num, info = {levels,
// chunk, workgroups, positions, positions that moved one by one}.  Returns the number of faults: a sentinel, a second visit, a
// piece outside its level, a misaligned group.
EMU_API long long emu_vg_walk(int Nz, int Nr, int Nc, int L, int swt, int do_app, long long* counts, long long* info) {
    Volume v(Nz, Nr, Nc, L, swt);
    v.fill(nullptr);
    for (int num = 0; num < v.nbands(); num++) counts[num] = 0;
    std::vector<std::vector<char>> seen;
    for (int l = 1; l <= L; l++) seen.emplace_back((size_t)v.level_n(l), 0);
    long long bad = 0, wrong = 0;
    for (int blk = 0; blk < v.blocks(); blk++)
        bad += v.walk(blk, do_app, [&](int l, long long i, int) {
            if (seen[l][(size_t)i]++) wrong++;
            const int nm = 7 + ((do_app && v.t.m[l][7]) ? 1 : 0);
            for (int k = 0; k < nm; k++) {
                const real_t x = v.t.m[l][k][i];
                if (x == kSentinel) wrong++;
                else counts[(int)x]++;
            }
        });
    long long singles = 0;
    for (int l = 0; l < L; l++)
        if (v.t.n[l] & 3) singles += v.t.n[l];
    info[0] = v.t.nlevels, info[1] = v.t.chunk, info[2] = v.blocks(), info[3] = v.total, info[4] = singles;
    return bad + wrong + v.touched();
}

// vol_group_soft_kernel on the caller's values (`flat`: the sub-bands one behind the other in `num` order, overwritten with the
// result); betas[l - 1]: the threshold of level l.  Returns the number of faults.
EMU_API long long emu_vg_soft(int Nz, int Nr, int Nc, int L, int swt, int do_app, const real_t* betas, real_t* flat) {
    Volume v(Nz, Nr, Nc, L, swt);
    v.fill(flat);
    long long bad = 0;
    for (int blk = 0; blk < v.blocks(); blk++)
        bad += v.walk(blk, do_app, [&](int l, long long i, int) {
            const int nm = 7 + ((do_app && v.t.m[l][7]) ? 1 : 0);
            VolSumSq ss = {real_t(0), real_t(0)};
            for (int k = 0; k < nm; k++) vol_sumsq_add(ss, v.t.m[l][k][i]);
            const real_t res = vol_group_res(ss, betas[l]);
            for (int k = 0; k < nm; k++) v.t.m[l][k][i] = v.t.m[l][k][i] * res;
        });
    v.read(flat);
    return bad + v.touched();
}

// vol_group_norm_kernel and vol_group_norm_final_kernel with their order of additions: a lane's own terms, the shuffle tree of
// each wavefront, the four wavefronts of a workgroup, then one wavefront over the partial sums.  Returns the number of faults.
EMU_API long long emu_vg_norm(int Nz, int Nr, int Nc, int L, int swt, int do_app, const real_t* flat, double* out) {
    Volume v(Nz, Nr, Nc, L, swt);
    v.fill(flat);
    auto tree = [](double* s) {  // 64 lanes, as __shfl_down leaves lane 0
        for (int off = 32; off > 0; off >>= 1)
            for (int lane = 0; lane < off; lane++) s[lane] += s[lane + off];
        return s[0];
    };
    long long bad = 0;
    std::vector<double> partial((size_t)v.blocks());
    for (int blk = 0; blk < v.blocks(); blk++) {
        double s[kVolGroupThreads] = {0};
        bad += v.walk(blk, do_app, [&](int l, long long i, int tid) {
            const int nm = 7 + ((do_app && v.t.m[l][7]) ? 1 : 0);
            double ss = 0.0;
            for (int k = 0; k < nm; k++) ss += vol_group_sq(v.t.m[l][k][i]);
            s[tid] += sqrt(ss);
        });
        double part[4];
        for (int w = 0; w < 4; w++) part[w] = tree(s + 64 * w);
        partial[(size_t)blk] = part[0] + part[1] + part[2] + part[3];
    }
    double s[64] = {0};
    for (int lane = 0; lane < 64; lane++)
        for (int i = lane; i < v.blocks(); i += 64) s[lane] += partial[(size_t)i];
    *out = tree(s);
    return bad + v.touched();
}

#ifdef EMU_VOLUME_GROUP_MAIN
// Stand-alone form for the sanitizer run: reads records {int64 Nz, Nr, Nc, L, swt, do_app, n; L betas; n values} from the file
// named first and writes what the group threshold leaves to the file named second; prints "walk-faults soft-faults norm-faults
// norm-as-hex-bits" per record.
#include <stdio.h>
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!f || !out) return 2;
    long long head[7];
    while (fread(head, sizeof(long long), 7, f) == 7) {
        const int Nz = (int)head[0], Nr = (int)head[1], Nc = (int)head[2], L = (int)head[3], swt = (int)head[4], do_app = (int)head[5];
        std::vector<real_t> betas((size_t)L), x((size_t)head[6]);
        if (fread(betas.data(), sizeof(real_t), betas.size(), f) != betas.size()) return 3;
        if (fread(x.data(), sizeof(real_t), x.size(), f) != x.size()) return 3;
        std::vector<long long> counts((size_t)(1 + 7 * L));
        long long info[5];
        const long long bad_walk = emu_vg_walk(Nz, Nr, Nc, L, swt, do_app, counts.data(), info);
        double norm = 0.0;
        const long long bad_norm = emu_vg_norm(Nz, Nr, Nc, L, swt, do_app, x.data(), &norm);
        const long long bad_soft = emu_vg_soft(Nz, Nr, Nc, L, swt, do_app, betas.data(), x.data());
        unsigned long long bits = 0;
        __builtin_memcpy(&bits, &norm, sizeof(norm));
        printf("%lld %lld %lld %llx\n", bad_walk, bad_soft, bad_norm, bits);
        if (fwrite(x.data(), sizeof(real_t), x.size(), out) != x.size()) return 3;
    }
    fclose(f);
    fclose(out);
    return 0;
}
#endif
