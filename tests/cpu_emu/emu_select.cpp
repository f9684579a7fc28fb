// emu_select.cpp -- the pass logic of pypwt_amd/csrc/select_kernels.hpp on the host (test-only; built by
// tests/test_emu_select.py with g++ -DPDWT_CPU_EMU, once more with -DPDWT_DOUBLE for the fp64 keys).
//
// The driver below does what the two kernels do between them -- a histogram of the pass's digit through select_classify, the
// partial sums, select_step -- with one "workgroup", so the digit, bucket-walk and two-rank logic run exactly as on the GPU.
#include "../../pypwt_amd/csrc/select_kernels.hpp"

#include <vector>

using namespace pdwt;

extern "C" __attribute__((visibility("default"))) int emu_select_passes(void) { return kSelectPasses; }

// median of |x[0 .. n)| (zeros left out when skip_zeros) and sigma = median / 0.6745; returns the hi_mode the walk ended in
extern "C" __attribute__((visibility("default"))) int emu_select_median(const real_t* x, long long n, int skip_zeros, double* median,
                                                                        double* sigma) {
    SelectState st = {};
    std::vector<unsigned> h(kSelectMaxBins), part(256), part16(16);
    for (int pass = 0; pass < kSelectPasses; pass++) {
        const int bits = select_pass_bits(pass), shift = select_pass_shift(pass), bins = 1 << bits;
        if (!(pass > 0 && st.empty)) {
            for (int b = 0; b < bins; b++) h[b] = 0;
            unsigned hi_min = st.hi_min;
            for (long long i = 0; i < n; i++) {
                const select_key_t key = select_key(x[i]);
                if (pass == 0 && key == 0) st.zeros++;
                const int d = select_classify(key, shift, bits, (select_key_t)st.lo_prefix, pass > 0 ? st.hi_mode : 0,
                                              (select_key_t)st.hi_prefix, &hi_min);
                if (d >= 0) h[d]++;
            }
            st.hi_min = hi_min;
        }
        for (int t = 0; t < 256; t++) part[t] = select_part_sum(h.data(), bins, t);
        for (int g = 0; g < 16; g++) part16[g] = select_part16_sum(part.data(), g);
        select_step(st, pass, h.data(), part.data(), part16.data(), n, skip_zeros);
    }
    *median = select_median(st);
    *sigma = *median / kSigmaDenominator;
    return st.hi_mode;
}

#ifdef EMU_SELECT_MAIN
// Stand-alone form for the sanitizer run: reads records {int64 n, int64 skip_zeros, n values} from the file named on the
// command line and prints one median per record as a hexadecimal double.
#include <stdio.h>
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long head[2];
    while (fread(head, sizeof(long long), 2, f) == 2) {
        std::vector<real_t> x((size_t)head[0]);
        if (head[0] > 0 && fread(x.data(), sizeof(real_t), x.size(), f) != x.size()) return 3;
        double median = 0, sigma = 0;
        emu_select_median(x.data(), head[0], (int)head[1], &median, &sigma);
        printf("%a\n", median);
    }
    fclose(f);
    return 0;
}
#endif
