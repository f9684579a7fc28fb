// emu_select_rank.cpp -- the rank logic of pypwt_amd/csrc/select_kernels.hpp (the K-th largest |c| over several bands) on the
// host (test-only; built by tests/test_emu_select_rank.py with g++ -DPDWT_CPU_EMU, once more with -DPDWT_DOUBLE).
//
// The driver does what select_hist_bands_kernel and select_walk_rank_kernel do between them: every pass, the SEVERAL disjoint
// ranges [starts[r], starts[r] + lens[r]) of x -- the pieces of the swept bands -- add their digits to ONE histogram through
// select_classify, then the partial sums and select_rank_step; select_rank_result after the last pass.
#include "../../pypwt_amd/csrc/select_kernels.hpp"

#include <vector>

using namespace pdwt;

extern "C" __attribute__((visibility("default"))) int emu_select_rank_passes(void) { return kSelectPasses; }

// *threshold = the K-th largest |x| over the ranges (as select_rank_value), *kept = elements at least that large; returns the
// number of histogram sweeps that ran (0 when K needs none)
extern "C" __attribute__((visibility("default"))) int emu_select_rank(const real_t* x, const long long* starts, const long long* lens,
                                                                      int nranges, long long k, real_t* threshold,
                                                                      unsigned long long* kept, unsigned long long* key_out) {
    unsigned long long n = 0;
    for (int r = 0; r < nranges; r++) n += (unsigned long long)lens[r];
    SelectState st = {};
    std::vector<unsigned> h(kSelectMaxBins), part(256), part16(16);
    int sweeps = 0;
    for (int pass = 0; pass < kSelectPasses; pass++) {
        const int bits = select_pass_bits(pass), shift = select_pass_shift(pass), bins = 1 << bits;
        for (int b = 0; b < kSelectMaxBins; b++) h[b] = 0;
        const bool skip = pass == 0 ? select_rank_flag(k, n) != 0 : st.empty != 0;
        if (!skip) {
            sweeps++;
            unsigned unused = kSelectNoDigit;
            for (int r = 0; r < nranges; r++)
                for (long long i = starts[r]; i < starts[r] + lens[r]; i++) {
                    const int d = select_classify(select_key(x[i]), shift, bits, (select_key_t)st.lo_prefix, 0, 0, &unused);
                    if (d >= 0) h[d]++;
                }
        }
        for (int t = 0; t < 256; t++) part[t] = select_part_sum(h.data(), bins, t);
        for (int g = 0; g < 16; g++) part16[g] = select_part16_sum(part.data(), g);
        select_rank_step(st, pass, h.data(), part.data(), part16.data(), k, n);
    }
    const select_key_t key = select_rank_result(st, k, n, kept);
    *threshold = select_rank_value(key);
    *key_out = key;
    return sweeps;
}

#ifdef EMU_SELECT_RANK_MAIN
// Stand-alone form for the sanitizer run: reads records {int64 n, int64 nranges, int64 k, nranges x (start, len), n values} from
// the file named on the command line and prints "threshold-as-hex-bits kept" per record.
#include <stdio.h>
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long head[3];
    while (fread(head, sizeof(long long), 3, f) == 3) {
        std::vector<long long> rg((size_t)(2 * head[1]));
        if (head[1] > 0 && fread(rg.data(), sizeof(long long), rg.size(), f) != rg.size()) return 3;
        std::vector<real_t> x((size_t)head[0]);
        if (head[0] > 0 && fread(x.data(), sizeof(real_t), x.size(), f) != x.size()) return 3;
        std::vector<long long> starts, lens;
        for (long long r = 0; r < head[1]; r++) {
            starts.push_back(rg[2 * r]);
            lens.push_back(rg[2 * r + 1]);
        }
        real_t t = 0;
        unsigned long long kept = 0, key = 0, bits = 0;
        emu_select_rank(x.data(), starts.data(), lens.data(), (int)head[1], head[2], &t, &kept, &key);
        __builtin_memcpy(&bits, &t, sizeof(t));
        printf("%llx %llu\n", bits, kept);
    }
    fclose(f);
    return 0;
}
#endif
