// emu_san.cpp -- stand-alone programs that run ONE family of the emulated tile functions under the address and undefined-behaviour
// sanitizers (tests/test_emu_sanitized.py and tests/test_emu_sanitized_more.py build one per family: -DEMU_SAN_FWDSTREAM, _INVSTREAM,
// _FUSED, _FAST, _SPLIT, _LONG; _TAIL, _PYRAMID, _FUSED1D, _WAVE, _RING, _REG1, _STREAM or _ROWS, with -DEMU_SLACK=0).  Only that family's kernel
// headers are compiled -- all of emu_kernels.cpp under the sanitizers takes longer to compile than a test may.  Nothing sanitised
// is loaded into python.  A program that serves several entry points (the tails, the pyramids, the wave kernels, the ring) takes
// which one as its record's first integer.
//
// Where the shared library's entry point packs several planes into one array (det = H|V|D of every level, l1 = H1|V1|D1, ...), the
// program calls the family's inner emu_*_planes function instead, with one block per plane: a read behind H1 lands in a redzone,
// not in V1.  The range-checked stores of the emulation (row_st4 / row_st8 / row_st16 / row_stn) abort on a store that is only
// partly in range.
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
#elif defined(EMU_SAN_TAIL)
#include "emu_tail.inc"
#elif defined(EMU_SAN_PYRAMID)
#include "emu_pyramid.inc"
#elif defined(EMU_SAN_FUSED1D)
#include "emu_dwt1_fused.inc"
#elif defined(EMU_SAN_WAVE)
#include "emu_wave.inc"
#elif defined(EMU_SAN_RING)
#include "emu_ring.inc"
#elif defined(EMU_SAN_REG1)
#include "emu_dwt1_reg.inc"
#elif defined(EMU_SAN_STREAM)
#include "emu_stream.inc"
#elif defined(EMU_SAN_ROWS)
#include "emu_swt_rows.inc"
#else
#error "name a family: -DEMU_SAN_FWDSTREAM, _INVSTREAM, _FUSED, _FAST, _SPLIT, _LONG, _TAIL, _PYRAMID, _FUSED1D, _WAVE, _RING, _REG1, _STREAM or _ROWS"
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
#elif defined(EMU_SAN_TAIL)
    if (ni < 1 || nf != 0) return -100;
    if (I[0] == 0) {
        // ints: 0, inverse, batch, R0, C0, K, hlen, threads, unrolled;  buffers: image, lo, hi, app, then H, V, D of each level
        if (ni != 9 || I[5] < 1 || nb != 4 + 3 * I[5]) return -100;
        return emu_dwt2_tail_planes((int)I[1], B[0], (int)I[2], (int)I[3], (int)I[4], (int)I[5], B[1], B[2], (int)I[6], (int)I[7], (int)I[8], B + 4, B[3]);
    }
    if (I[0] == 1) {
        // ints: 1, inverse, batch, Nr, Nc, L, hlen;  buffers: image, lo, hi, beta (or null), app, then H, V, D of each level
        if (ni != 7 || I[5] < 1 || nb != 5 + 3 * I[5]) return -100;
        return emu_swt2_tail_planes((int)I[1], B[0], (int)I[2], (int)I[3], (int)I[4], (int)I[5], B[1], B[2], (int)I[6], B[3], B + 5, B[4]);
    }
    // ints: 2, inverse, rows, N0, K, G, hlen, unrolled;  buffers: data, lo, hi, app, then D of each level
    if (ni != 8 || I[4] < 1 || nb != 4 + I[4]) return -100;
    return emu_dwt1_rows_tail_planes((int)I[1], B[0], (int)I[2], (int)I[3], (int)I[4], (int)I[5], B[1], B[2], (int)I[6], (int)I[7], B + 4, B[3]);
#elif defined(EMU_SAN_PYRAMID)
    if (ni < 1 || nf != 0) return -100;
    if (I[0] == 0) {
        // ints: 0, batch, N0r, N0c, hlen, tile;  buffers: in, lo, hi, H1, V1, D1, A2, H2, V2, D2
        if (ni != 6 || nb != 10) return -100;
        return emu_dwt2_fwd_pyr2_planes(B[0], (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], B + 3, B + 6);
    }
    if (I[0] == 1) {
        // ints: 1, batch, N0r, N0c, hlen, tile;  buffers: H1, V1, D1, A2, H2, V2, D2, lo, hi, out
        if (ni != 6 || nb != 10) return -100;
        return emu_dwt2_inv_pyr2_planes(B, B + 3, (int)I[1], (int)I[2], (int)I[3], B[7], B[8], (int)I[4], (int)I[5], B[9]);
    }
    // ints: 2, inverse, batch, N0r, N0c, hlen, tile;  buffers: image, lo, hi, app, then H, V, D of levels 1, 2, 3
    if (ni != 7 || nb != 13) return -100;
    return emu_dwt2_pyr3_planes((int)I[1], B[0], (int)I[2], (int)I[3], (int)I[4], B[1], B[2], (int)I[5], (int)I[6], B + 4, B[3]);
#elif defined(EMU_SAN_FUSED1D)
    // ints: inverse, rows, N0, K, hlen, small;  buffers: io, lo, hi, app, then D of each level
    if (ni != 6 || nf != 0 || I[3] < 1 || nb != 4 + I[3]) return -100;
    return emu_dwt1_fused_planes((int)I[0], B[0], (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], B + 4, B[3]);
#elif defined(EMU_SAN_WAVE)
    if (ni < 1 || nf != 0) return -100;
    if (I[0] == 0) {
        // ints: 0, batch, Nr, Nc, hlen, seg_out, guard;  buffers: in, lo, hi, A, H, V, D
        if (ni != 7 || nb != 7) return -100;
        return emu_dwt2_fwd_wave(B[0], (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], (int)I[6], B[3], B[4], B[5], B[6]);
    }
    if (I[0] == 1) {
        // ints: 1, batch, Nrc, Ncc, Nr, Nc, hlen, seg_pairs, guard;  buffers: A, H, V, D, lo, hi, out
        if (ni != 9 || nb != 7) return -100;
        return emu_dwt2_inv_wave(B[0], B[1], B[2], B[3], (int)I[1], (int)I[2], (int)I[3], (int)I[4], (int)I[5], B[4], B[5], (int)I[6], (int)I[7], (int)I[8], B[6]);
    }
    // ints: 2, batch, N0r, N0c, hlen, seg2_out;  buffers: in, lo, hi, H1, V1, D1, A2, H2, V2, D2
    if (ni != 6 || nb != 10) return -100;
    return emu_dwt2_fwd2_wave_planes(B[0], (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], B + 3, B + 6);
#elif defined(EMU_SAN_RING)
    if (ni < 1 || nf != 0 || nb != 7) return -100;
    if (I[0] == 0) {
        // ints: 0, batch, Nr, Nc, hlen, seg_out, cpl;  buffers: in, lo, hi, A, H, V, D
        if (ni != 7) return -100;
        return emu_dwt2_fwd_ring(B[0], (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], (int)I[6], B[3], B[4], B[5], B[6]);
    }
    // ints: 1, batch, Nrc, Ncc, Nr, Nc, hlen, seg_pairs, cpl;  buffers: A, H, V, D, lo, hi, out
    if (ni != 9) return -100;
    return emu_dwt2_inv_ring(B[0], B[1], B[2], B[3], (int)I[1], (int)I[2], (int)I[3], (int)I[4], (int)I[5], B[4], B[5], (int)I[6], (int)I[7], (int)I[8], B[6]);
#elif defined(EMU_SAN_REG1)
    // ints: inverse, rows, N0, K, hlen, bpw;  buffers: forward in, lo, hi, app, then D of each level;  inverse app, lo, hi, out, then D ...
    if (ni != 6 || nf != 0 || I[3] < 1 || nb != 4 + I[3]) return -100;
    if (!I[0]) return emu_dwt1_fwd_reg_planes(B[0], (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], B + 4, B[3]);
    return emu_dwt1_inv_reg_planes(B[0], B + 4, (int)I[1], (int)I[2], (int)I[3], B[1], B[2], (int)I[4], (int)I[5], B[3]);
#elif defined(EMU_SAN_STREAM)
    if (ni < 1 || nb != 7) return -100;
    if (I[0] == 0) {
        // ints: 0, inverse, batch, Nr, Nc, level, hlen, R;  floats: soft threshold;  buffers: io, lo, hi, A, H, V, D
        if (ni != 8 || nf != 1) return -100;
        return emu_swt2_stream((int)I[1], B[0], (int)I[2], (int)I[3], (int)I[4], (int)I[5], B[1], B[2], (int)I[6], F[0], B[3], B[4], B[5], B[6], (int)I[7]);
    }
    // ints: 1, inverse, batch, Nr, Nc, hlen, R;  buffers: io, lo, hi, A, H, V, D
    if (ni != 7 || nf != 0) return -100;
    return emu_dwt2_stream((int)I[1], B[0], (int)I[2], (int)I[3], (int)I[4], B[1], B[2], (int)I[5], (int)I[6], B[3], B[4], B[5], B[6]);
#elif defined(EMU_SAN_ROWS)
    // ints: inverse, Nr, Nc, level, hlen;  buffers: in0, in1 (or null: forward), lo, hi, out0, out1 (or null: inverse)
    if (ni != 5 || nf != 0 || nb != 6) return -100;
    return emu_swt1_split((int)I[0], B[0], B[1], (int)I[1], (int)I[2], (int)I[3], B[2], B[3], (int)I[4], B[4], B[5]);
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
