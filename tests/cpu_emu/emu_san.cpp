// emu_san.cpp -- stand-alone programs that run ONE family of the emulated tile functions under the address and undefined-behaviour
// sanitizers (tests/test_emu_sanitized.py builds one per family: -DEMU_SAN_FWDSTREAM, _INVSTREAM, _FUSED, _FAST, _SPLIT or _LONG, with
// -DEMU_SLACK=0).  Only that family's kernel headers are compiled -- all of emu_kernels.cpp under the sanitizers takes longer to
// compile than a test may.  Nothing sanitised is loaded into python.
//
// argv[1] holds records, argv[2] receives the outputs back to back.  A record:
//   int64 nint, int64 ints[nint]      the family's integer arguments
//   int64 nflt, float flts[nflt]      its scalar float arguments
//   int64 nbuf, then per buffer  int64 n, int64 kind  [, float data[n] when kind == 0]
// kind 0 is an input, 1 an output; n < 0 is a null pointer.  Every buffer -- planes and filter taps alike -- is a malloc block of
// exactly n floats, outputs start as NaN, and the emulated LDS is the geometry's size to the element (EMU_SLACK = 0): a read or a
// write one element outside what the kernel is entitled to touches a redzone.
#include <stdio.h>

#if defined(EMU_SAN_FWDSTREAM)
#include "emu_swt_fwdstream.inc"
#elif defined(EMU_SAN_INVSTREAM)
#include "emu_swt_invstream.inc"
#elif defined(EMU_SAN_FUSED)
#include "emu_swt_fused.inc"
#elif defined(EMU_SAN_FAST)
#include "emu_dwt2_fast.inc"
#elif defined(EMU_SAN_SPLIT)
#include "emu_swt_split.inc"
#elif defined(EMU_SAN_LONG)
#include "emu_dwt2_long.inc"
#else
#error "name a family: -DEMU_SAN_FWDSTREAM, _INVSTREAM, _FUSED, _FAST, _SPLIT or _LONG"
#endif

static_assert(EMU_SLACK == 0, "the sanitizer programs size the emulated LDS exactly");

// the family's entry point on a record's arguments; returns its status, or -100 for a malformed record
static int call(const long long* I, int ni, const float* F, int nf, float** B, int nb) {
#if defined(EMU_SAN_FWDSTREAM)
    // ints: batch, Nr, Nc, level, hlen, seg;  buffers: in, lo, hi, A, H, V, D
    if (ni != 6 || nf != 0 || nb != 7) return -100;
    return emu_swt2_fwdstream(B[0], (int)I[0], (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], B[3], B[4], B[5], B[6]);
#elif defined(EMU_SAN_INVSTREAM)
    // ints: batch, Nr, Nc, level, hlen, seg;  floats: beta;  buffers: A, H, V, D, lo, hi, out
    if (ni != 6 || nf != 1 || nb != 7) return -100;
    return emu_swt2_invstream(B[0], B[1], B[2], B[3], (int)I[0], (int)I[1], (int)I[2], (int)I[3], B[4], B[5], (int)I[4], F[0], (int)I[5], B[6]);
#elif defined(EMU_SAN_FUSED)
    // ints: taps (2 or 4), batch, Nr, Nc, K, f0, seg, inverse, cpl;  buffers: in, det, out, lo, hi, beta (or null)
    if (ni != 9 || nf != 0 || nb != 6) return -100;
    if (I[0] == 2) return emu_swt2_fused(B[0], B[1], B[2], (int)I[1], (int)I[2], (int)I[3], (int)I[4], (int)I[5], (int)I[6], B[3], B[4], B[5], (int)I[7], (int)I[8]);
    return emu_swt4_fused(B[0], B[1], B[2], (int)I[1], (int)I[2], (int)I[3], (int)I[5], (int)I[6], B[3], B[4], B[5], (int)I[7]);
#elif defined(EMU_SAN_FAST)
    // ints: inverse, batch, Nr, Nc, hlen, tile;  buffers: forward in, lo, hi, A, H, V, D;  inverse A, H, V, D, lo, hi, out
    if (ni != 6 || nf != 0 || nb != 7) return -100;
    const int Nr = (int)I[2], Nc = (int)I[3];
    if (!I[0]) return emu_dwt2_fwd_fast(B[0], (int)I[1], Nr, Nc, B[1], B[2], (int)I[4], (int)I[5], B[3], B[4], B[5], B[6]);
    return emu_dwt2_inv_fast(B[0], B[1], B[2], B[3], (int)I[1], (Nr + 1) / 2, (Nc + 1) / 2, Nr, Nc, B[4], B[5], (int)I[4], (int)I[5], B[6]);
#elif defined(EMU_SAN_SPLIT)
    // ints: inverse, batch, Nr, Nc, level, hlen, seg (rows of a chain per segment of the strip walk, 0: two segments);  floats: beta;
    // buffers: io, lo, hi, A, H, V, D.  The column pass must have gone through swt_colstream_kernels.hpp: -101 otherwise
    if (ni != 7 || nf != 1 || nb != 7) return -100;
    char seg[32];
    snprintf(seg, sizeof(seg), "%d", (int)I[6]);
    setenv("EMU_SPLIT_COLSTREAM", "1", 1);
    if (I[6] > 0) setenv("EMU_COLSTREAM_SEG", seg, 1);
    else unsetenv("EMU_COLSTREAM_SEG");
    const int before = emu_colstream_runs();
    const int rc = emu_swt2_split((int)I[0], B[0], (int)I[1], (int)I[2], (int)I[3], (int)I[4], B[1], B[2], (int)I[5], F[0], B[3], B[4], B[5], B[6]);
    return rc == 0 && emu_colstream_runs() != before + 1 ? -101 : rc;
#elif defined(EMU_SAN_LONG)
    // ints: inverse, batch, Nr, Nc, hlen, seg, shape;  buffers: forward in, lo, hi, A, H, V, D;  inverse A, H, V, D, lo, hi, out
    if (ni != 7 || nf != 0 || nb != 7) return -100;
    const int Nr = (int)I[2], Nc = (int)I[3];
    if (!I[0]) return emu_dwt2_fwd_long(B[0], (int)I[1], Nr, Nc, B[1], B[2], (int)I[4], (int)I[5], (int)I[6], B[3], B[4], B[5], B[6]);
    return emu_dwt2_inv_long(B[0], B[1], B[2], B[3], (int)I[1], Nr / 2, Nc / 2, Nr, Nc, B[4], B[5], (int)I[4], (int)I[5], (int)I[6], B[6]);
#endif
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    enum { MAXN = 16 };
    long long n = 0, I[MAXN];
    float F[MAXN];
    int records = 0;
    while (fread(&n, sizeof(n), 1, f) == 1) {
        const int ni = (int)n;
        if (ni < 0 || ni > MAXN || fread(I, sizeof(long long), ni, f) != (size_t)ni) return 3;
        if (fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > MAXN || fread(F, sizeof(float), (size_t)n, f) != (size_t)n) return 3;
        const int nf = (int)n;
        if (fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > MAXN) return 3;
        const int nb = (int)n;
        float* B[MAXN];
        long long len[MAXN], kind[MAXN];
        for (int b = 0; b < nb; b++) {
            if (fread(&len[b], sizeof(long long), 1, f) != 1 || fread(&kind[b], sizeof(long long), 1, f) != 1) return 3;
            B[b] = len[b] < 0 ? nullptr : (float*)malloc(sizeof(float) * (size_t)len[b]);
            if (len[b] < 0) continue;
            if (kind[b] == 0) { if (fread(B[b], sizeof(float), (size_t)len[b], f) != (size_t)len[b]) return 3; }
            else memset(B[b], 0xff, sizeof(float) * (size_t)len[b]);  // NaN
        }
        const int rc = call(I, ni, F, nf, B, nb);
        if (rc != 0) { fprintf(stderr, "record %d: status %d\n", records, rc); return 4; }
        for (int b = 0; b < nb; b++) {
            if (len[b] >= 0 && kind[b] == 1 && fwrite(B[b], sizeof(float), (size_t)len[b], g) != (size_t)len[b]) return 5;
            free(B[b]);
        }
        records++;
    }
    fclose(f);
    if (fclose(g) != 0) return 5;
    printf("%d\n", records);
    return 0;
}
