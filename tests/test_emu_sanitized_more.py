"""The kernel families that take planes of any size -- the whole-transform-in-one-workgroup tails, the pyramids, the fused 1D
pyramid, the wave kernels with their guards, the register ring, the 1D transform in registers, the any-length stream kernels, the
a-trous row kernels -- under the address and undefined-behaviour sanitizers, as tests/test_emu_sanitized.py does for the families
that load 16-byte groups at 4-byte alignment.

tests/cpu_emu/emu_san.cpp is built once per family as a stand-alone program (-DEMU_SLACK=0: the emulated LDS is what the launcher
asks for, to the element).  Where the shared library's entry point packs several planes into one array (det = H|V|D of every
level, l1 = H1|V1|D1, l2 = A2|H2|V2|D2), the program calls the family's inner function with one heap block of exactly its size
per plane: a read behind H1 ends in a redzone, not in V1.  The emulation's range-checked row stores abort on a store that is only
partly in range.  Each test computes the outputs with the unsanitised shared library, runs the program once with
ASAN_OPTIONS=detect_leaks=1 and UBSAN_OPTIONS=halt_on_error=1, requires exit status 0 and the program's outputs bit-equal to the
library's with no NaN left in any of them.  Nothing sanitised is loaded into python.

A combination the emulation's entry point declines (status -2) has nothing to run; each test counts them, states which they are,
and declines no more than half of its grid.
"""
import ctypes as C

import numpy as np
import pytest

from emu_san_util import IN, OUT, compile_programs
from emu_san_util import nan as _nan
from emu_san_util import plane as _plane
from emu_san_util import run as _run
from emu_util import P, lib
from oracle import oracle

# family -> what selects it and the filter lengths its program instantiates (the cases below use no other)
FAMILIES = {
    "tail": ["-DEMU_SAN_TAIL", "-DEMU_TAIL_HLENS(X)=X(2) X(4) X(8)", "-DEMU_ROWS_TAIL_HLENS(X)=X(2) X(8)"],
    "pyramid": ["-DEMU_SAN_PYRAMID", "-DEMU_PYR_HLENS(X)=X(2) X(8) X(16)"],
    "fused1d": ["-DEMU_SAN_FUSED1D", "-DEMU_FUSED1D_HLENS(X)=X(2) X(8) X(20)"],
    "wave": ["-DEMU_SAN_WAVE"],
    "ring": ["-DEMU_SAN_RING", "-DEMU_RING_HLENS(X)=X(10) X(16) X(20)"],
    "reg1": ["-DEMU_SAN_REG1", "-DEMU_REG1_HLENS(X)=X(2) X(8) X(20)"],
    "stream": ["-DEMU_SAN_STREAM"],
    "rows": ["-DEMU_SAN_ROWS", "-DEMU_SWT_ROWS_HLENS(X)=X(4) X(10) X(20)"],
}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """Every family's program, compiled side by side (emu_san_util.compile_programs); family -> a function returning its path."""
    get, finish = compile_programs(tmp_path_factory.mktemp("emu_san_more"), FAMILIES)
    yield get
    finish()


def _split(flat, sizes):
    """The planes packed back to back in flat, as views of it."""
    assert flat.ndim == 1 and flat.size == sum(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [flat[offs[i]:offs[i + 1]] for i in range(len(sizes))]


def _halve(n):
    return (n + 1) // 2


# ----------------------------------------------------------------------------- tails
def test_dwt2_tail_of_all_remaining_levels_under_sanitizers(programs, tmp_path):
    """dwt2_tail_kernels.hpp: every R0 x C0 of {5 ... 12, 31, 33} x {6 ... 13, 32, 35}, one to three levels, 2, 4, 8 and 12 taps
    (down to 1 x 1 planes: the periodic index wraps more than once), 64, 256 and 1024 threads, the unrolled and the run-time filter
    length, the power-of-two sizes through the mask / shift kernels and (unrolled = 2) through the general ones, both directions,
    one and two images.  Declined: 64 threads on images of more than 64 x 16 samples (33 x 32, 31 x 35, 33 x 35)."""
    L = lib()
    cases, declined, total = [], set(), 0
    for wname in ("haar", "db2", "db4", "db6"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for R0 in list(range(5, 13)) + [31, 33]:
            for C0 in list(range(6, 14)) + [32, 35]:
                pow2 = (R0 & (R0 - 1)) == 0 and (C0 & (C0 - 1)) == 0
                for K in (1, 2, 3):
                    B = 1 + (R0 + C0 + K) % 2
                    dims = [(R0, C0)]
                    for _ in range(K):
                        dims.append((_halve(dims[-1][0]), _halve(dims[-1][1])))
                    sizes = [B * r * c for r, c in dims[1:] for _ in range(3)]
                    x = _plane((B, R0, C0), 7700)
                    det_in = _plane((sum(sizes),), 7710 + K, signed=True)
                    app_in = _plane((B,) + dims[-1], 7720 + K, signed=True)
                    # unrolled: 0 run-time length, 1 compile-time (2 ... 8 taps; 12 taps run through the run-time length either way),
                    # 2 the general kernels at a power-of-two size
                    for unrolled in ((0, 1) if hlen <= 8 else (1,)) + ((2,) if pow2 else ()):
                        for threads in (64, 256, 1024):
                            total += 2
                            det, app = _nan(sum(sizes)), _nan((B,) + dims[-1])
                            rc = L.emu_dwt2_tail(0, P(x), B, R0, C0, K, P(dlo), P(dhi), hlen, threads, unrolled, P(det), P(app))
                            if rc == -2:
                                declined.add((threads, R0, C0))
                                continue
                            assert rc == 0, (wname, R0, C0, K, threads, unrolled, rc)
                            cases.append(([0, 0, B, R0, C0, K, hlen, threads, unrolled], [],
                                          [(x, IN), (dlo, IN), (dhi, IN), (app, OUT)] + [(p, OUT) for p in _split(det, sizes)]))
                            out = _nan((B, R0, C0))
                            assert L.emu_dwt2_tail(1, P(out), B, R0, C0, K, P(rlo), P(rhi), hlen, threads, unrolled, P(det_in), P(app_in)) == 0
                            cases.append(([0, 1, B, R0, C0, K, hlen, threads, unrolled], [],
                                          [(out, OUT), (rlo, IN), (rhi, IN), (app_in, IN)] + [(p, IN) for p in _split(det_in, sizes)]))
    assert declined == {(64, 33, 32), (64, 31, 35), (64, 33, 35)}
    assert len(cases) > 12000 and 2 * (total - len(cases)) <= total
    _run(programs("tail"), tmp_path, cases)


def test_swt2_tail_whole_transform_of_tiny_images_under_sanitizers(programs, tmp_path):
    """swt2_tail_kernels.hpp: every Nr x Nc of 2 ... 17 and 64 x 64, one to three levels (dilations above the image size: the periodic
    index wraps several times), haar / db2 / db4, one and two images (which pick the launcher's shapes: one wavefront, 256 threads
    with 4 and with 16 staging trips), the inverse with and without the pending soft threshold, the power-of-two sizes through the
    mask / shift kernels and (a negative first threshold) through the general ones.  Nothing is declined."""
    L = lib()
    cases = []
    for wname in ("haar", "db2", "db4"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for Nr, Nc in [(r, c) for r in range(2, 18) for c in range(2, 18)] + [(64, 64)]:
            pow2 = (Nr & (Nr - 1)) == 0 and (Nc & (Nc - 1)) == 0
            n = Nr * Nc
            for lv in (1, 2, 3):
                for B in (1, 2):
                    sizes = [B * n] * (3 * lv)
                    x = _plane((B, Nr, Nc), 7800)
                    det, app = _nan(3 * lv * B * n), _nan((B, Nr, Nc))
                    assert L.emu_swt2_tail(0, P(x), B, Nr, Nc, lv, P(dlo), P(dhi), hlen, None, P(det), P(app)) == 0
                    cases.append(([1, 0, B, Nr, Nc, lv, hlen], [],
                                  [(x, IN), (dlo, IN), (dhi, IN), (None, IN), (app, OUT)] + [(p, OUT) for p in _split(det, sizes)]))
                    det_in = _plane((3 * lv * B * n,), 7810 + lv, signed=True)
                    app_in = _plane((B, Nr, Nc), 7820 + lv, signed=True)
                    betas = [None, np.array([0.3, 0.2, 0.1][:lv], dtype=np.float32)]
                    betas += [np.array([-1.0, 0.2, 0.1][:lv], dtype=np.float32)] if pow2 else []
                    for beta in betas:
                        out = _nan((B, Nr, Nc))
                        assert L.emu_swt2_tail(1, P(out), B, Nr, Nc, lv, P(rlo), P(rhi), hlen, None if beta is None else P(beta),
                                               P(det_in), P(app_in)) == 0
                        cases.append(([1, 1, B, Nr, Nc, lv, hlen], [],
                                      [(out, OUT), (rlo, IN), (rhi, IN), (beta, IN), (app_in, IN)] + [(p, IN) for p in _split(det_in, sizes)]))
    assert len(cases) >= 3 * 257 * 3 * 2 * 3
    _run(programs("tail"), tmp_path, cases)


def test_dwt1_rows_tail_under_sanitizers(programs, tmp_path):
    """dwt1_rows_kernels.hpp: rows of 8, 16, 24, 64 and 1024 / G samples (G = 3: 336), G = 1, 3 and the most rows that fit 1024 samples,
    a last group with fewer rows (one more row than two groups; a single row), every level count whose 2^K divides the row, up to the
    kernels' eight (levels shorter than the filter: the wrap goes around more than once), 2 and 8 taps unrolled and at run-time
    length, 20 taps at run-time length, both directions.  Declined: the first level count of each row length that does not divide it
    (or is above eight levels), which is asked for once per combination."""
    L = lib()
    cases, declined, total = [], set(), 0
    for wname in ("haar", "db4", "db10"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for N0base in (8, 16, 24, 64, 0):
            for Gsel in (1, 3, 0):
                if not N0base and not Gsel:
                    continue
                G = Gsel if Gsel else 1024 // N0base
                N0 = N0base if N0base else (1024 // G) & ~7  # (1024 / 3: the 336 samples below it, whole 16-sample groups)
                kmax = max(K for K in range(1, 9) if N0 % (1 << K) == 0)
                for rows in (2 * G + 1, 1):
                    for K in range(1, kmax + 2):
                        for unrolled in (0, 1) if hlen <= 8 else (0,):
                            total += 2
                            sizes = [rows * (N0 >> k) for k in range(1, K + 1)]
                            x = _plane((rows, N0), 7900)
                            det, app = _nan(sum(sizes)), _nan((rows, N0 >> K))
                            rc = L.emu_dwt1_rows_tail(0, P(x), rows, N0, K, G, P(dlo), P(dhi), hlen, unrolled, P(det), P(app))
                            assert rc == (0 if K <= kmax else -2), (wname, N0, G, rows, K, rc)
                            if rc == -2:
                                declined.add((N0, K))
                                continue
                            cases.append(([2, 0, rows, N0, K, G, hlen, unrolled], [],
                                          [(x, IN), (dlo, IN), (dhi, IN), (app, OUT)] + [(p, OUT) for p in _split(det, sizes)]))
                            det_in = _plane((sum(sizes),), 7910 + K, signed=True)
                            app_in = _plane((rows, N0 >> K), 7920 + K, signed=True)
                            out = _nan((rows, N0))
                            assert L.emu_dwt1_rows_tail(1, P(out), rows, N0, K, G, P(rlo), P(rhi), hlen, unrolled, P(det_in), P(app_in)) == 0
                            cases.append(([2, 1, rows, N0, K, G, hlen, unrolled], [],
                                          [(out, OUT), (rlo, IN), (rhi, IN), (app_in, IN)] + [(p, IN) for p in _split(det_in, sizes)]))
    assert declined == {(8, 4), (16, 5), (24, 4), (64, 7), (336, 5), (1024, 9)}
    assert any(c[0][3] == 1024 and c[0][4] == 8 for c in cases) and 2 * (total - len(cases)) <= total
    _run(programs("tail"), tmp_path, cases)


# ----------------------------------------------------------------------------- pyramids
def test_dwt2_two_level_pyramids_under_sanitizers(programs, tmp_path):
    """dwt2_pyramid_kernels.hpp, forward and inverse: every N0r x N0c of 4 ... 72 (steps of 4) x 8 ... 136 (steps of 8) -- rows of
    eight but not sixteen samples, ragged last tiles, second levels of 1 x 2 samples under 16 taps --, both tile shapes, 2, 8 and 16
    taps, one and two images.  Nothing is declined."""
    L = lib()
    cases = []
    for wname in ("haar", "db4", "db8"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for N0r in range(4, 73, 4):
            for N0c in range(8, 137, 8):
                B = 1 + (N0r // 4 + N0c // 8) % 2
                n1, n2 = (B, N0r // 2, N0c // 2), (B, N0r // 4, N0c // 4)
                s1, s2 = [int(np.prod(n1))] * 3, [int(np.prod(n2))] * 4
                x = _plane((B, N0r, N0c), 8000)
                l1_in, l2_in = _plane((sum(s1),), 8010, signed=True), _plane((sum(s2),), 8020, signed=True)
                for tile in (0, 1):
                    l1, l2 = _nan(sum(s1)), _nan(sum(s2))
                    assert L.emu_dwt2_fwd_pyr2(P(x), B, N0r, N0c, P(dlo), P(dhi), hlen, tile, P(l1), P(l2)) == 0
                    cases.append(([0, B, N0r, N0c, hlen, tile], [], [(x, IN), (dlo, IN), (dhi, IN)] +
                                  [(p, OUT) for p in _split(l1, s1) + _split(l2, s2)]))
                    out = _nan((B, N0r, N0c))
                    assert L.emu_dwt2_inv_pyr2(P(l1_in), P(l2_in), B, N0r, N0c, P(rlo), P(rhi), hlen, tile, P(out)) == 0
                    cases.append(([1, B, N0r, N0c, hlen, tile], [], [(p, IN) for p in _split(l1_in, s1) + _split(l2_in, s2)] +
                                  [(rlo, IN), (rhi, IN), (out, OUT)]))
    assert len(cases) == 3 * 18 * 17 * 2 * 2
    _run(programs("pyramid"), tmp_path, cases)


def test_dwt2_three_level_pyramid_under_sanitizers(programs, tmp_path):
    """dwt2_pyr3_kernels.hpp, forward and inverse: every N0r x N0c of 8 ... 136 in steps of 8 with 8 taps (ragged last tiles in both
    directions, every residue of the three tile sizes); with 2 and 16 taps (third levels of one sample under 16 taps) the square
    sizes, 8 rows or 8 columns against every other size, and every pair that adds up to 144; tiles of 2, 4 and 8 samples of the third
    level, one and two images.  Nothing is declined."""
    L = lib()
    full = [(r, c) for r in range(8, 137, 8) for c in range(8, 137, 8)]
    edge = [(r, c) for r, c in full if r == c or r == 8 or c == 8 or r + c == 144]
    cases = []
    for wname, sizes in (("haar", edge), ("db4", full), ("db8", edge)):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for N0r, N0c in sizes:
            B = 1 + (N0r // 8 + N0c // 8) % 2
            sz = [B * (N0r >> k) * (N0c >> k) for k in (1, 2, 3) for _ in range(3)]
            x = _plane((B, N0r, N0c), 8100)
            det_in, app_in = _plane((sum(sz),), 8110, signed=True), _plane((B, N0r // 8, N0c // 8), 8120, signed=True)
            for tile in (2, 4, 8):
                det, app = _nan(sum(sz)), _nan((B, N0r // 8, N0c // 8))
                assert L.emu_dwt2_pyr3(0, P(x), B, N0r, N0c, P(dlo), P(dhi), hlen, tile, P(det), P(app)) == 0
                cases.append(([2, 0, B, N0r, N0c, hlen, tile], [], [(x, IN), (dlo, IN), (dhi, IN), (app, OUT)] + [(p, OUT) for p in _split(det, sz)]))
                out = _nan((B, N0r, N0c))
                assert L.emu_dwt2_pyr3(1, P(out), B, N0r, N0c, P(rlo), P(rhi), hlen, tile, P(det_in), P(app_in)) == 0
                cases.append(([2, 1, B, N0r, N0c, hlen, tile], [], [(out, OUT), (rlo, IN), (rhi, IN), (app_in, IN)] + [(p, IN) for p in _split(det_in, sz)]))
    assert len(full) == 17 * 17 and len(edge) >= 17 * 4 - 6 and len(cases) == (len(full) + 2 * len(edge)) * 3 * 2
    _run(programs("pyramid"), tmp_path, cases)


def test_dwt1_fused_pyramid_under_sanitizers(programs, tmp_path):
    """dwt1_fused_kernels.hpp, forward and inverse: two to four levels of rows of 16 ... 1200 samples in steps of 2^K (every other
    one is whole 2^(K+1) samples and runs: alternately rows of half the alignment, 2^(K+1) but not 2^(K+2), and aligned ones) and of
    8224 and 8240 samples (a second tile of the inverse's 8192 samples), both tile sizes, 2, 8 and 20 taps (deepest levels of one or
    two samples), one and two rows.  Declined: the rows that are not whole 2^(K+1) samples, and one level (asked for on rows of 16, 20
    and 1200 samples): the kernels are written for two and more, which is all the launcher sends them -- with one level the forward
    staged 16-B groups from an origin that is not 4-aligned (8 taps, 16 samples: it read two samples behind the row) and the inverse
    wrote its last 8-sample block four samples behind a row of 20."""
    L = lib()
    cases, declined, total = [], 0, 0
    for wname in ("haar", "db4", "db10"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for K in (1, 2, 3, 4):
            for N0 in (16, 20, 1200) if K == 1 else list(range(16, 1201, 1 << K)) + [8224, 8240]:
                rows = 1 + (N0 >> (K + 1)) % 2
                sizes = [rows * (N0 >> k) for k in range(1, K + 1)]
                x = _plane((rows, N0), 8200)
                det_in, app_in = _plane((sum(sizes),), 8210 + K, signed=True), _plane((rows, N0 >> K), 8220 + K, signed=True)
                for small in (0, 1):
                    total += 2
                    want = -2 if K == 1 or N0 % (2 << K) else 0
                    det, app = _nan(sum(sizes)), _nan((rows, N0 >> K))
                    rc = L.emu_dwt1_fused(0, P(x), rows, N0, K, P(dlo), P(dhi), hlen, small, P(det), P(app))
                    out = _nan((rows, N0))
                    rci = L.emu_dwt1_fused(1, P(out), rows, N0, K, P(rlo), P(rhi), hlen, small, P(det_in), P(app_in))
                    assert rc == want and rci == want, (wname, N0, K, small, rc, rci)
                    if want:
                        declined += 2
                        continue
                    cases.append(([0, rows, N0, K, hlen, small], [], [(x, IN), (dlo, IN), (dhi, IN), (app, OUT)] + [(p, OUT) for p in _split(det, sizes)]))
                    cases.append(([1, rows, N0, K, hlen, small], [], [(out, OUT), (rlo, IN), (rhi, IN), (app_in, IN)] + [(p, IN) for p in _split(det_in, sizes)]))
    # per filter, tile size and direction: 3 rows of K = 1; 148 (K = 2), 74 (K = 3) and 38 + 1 (K = 4: 8240 too) of the others
    assert declined == 3 * 2 * 2 * (3 + 148 + 74 + 39) and 2 * declined <= total
    _run(programs("fused1d"), tmp_path, cases)


# ----------------------------------------------------------------------------- wave kernels
WAVE_WNAMES = ("haar", "db2", "db3", "db4")
# guard = 0 (direction, taps, rows per segment): segments that are not whole groups of the filter length's row pattern
WAVE_DECLINED = {(0, 6, 4), (0, 6, 8), (0, 8, 6), (1, 2, 6), (1, 4, 6), (1, 6, 4), (1, 6, 8), (1, 8, 6)}


def test_dwt2_wave_level_kernels_under_sanitizers(programs, tmp_path):
    """dwt2_wave_kernels.hpp, forward and inverse.  guard = 1: 4 ... 24 columns in steps of 4 and 252, 256, 260 (a ragged last strip
    of one group, whole strips, one group into the next strip), 5, 6, 33 and 64 rows (odd and even; planes shorter than the filter
    on both axes), segments that do and do not divide the output rows, one and two images, 2 ... 8 taps.  guard = 0 (the
    predicate-free variant) at 256 columns and 48 rows with segments of 4, 6, 8, 12 and 24 rows.  Declined: guard = 0 with segments
    that are not whole groups of the filter length's row pattern (WAVE_DECLINED: 6 taps with 4 and 8 rows, 8 taps with 6, the
    inverse of 2 and 4 taps with 6)."""
    L = lib()
    cases, declined, total = [], set(), 0
    for wname in WAVE_WNAMES:
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        grid = [(1, Nr, Nc, seg) for Nc in list(range(4, 25, 4)) + [252, 256, 260] for Nr in (5, 6, 33, 64) for seg in (4, 5, (Nr + 1) // 2)]
        grid += [(0, 48, 256, seg) for seg in (4, 6, 8, 12, 24)]
        for guard, Nr, Nc, seg in grid:
            for B in (1, 2):
                total += 2
                r2, c2 = (Nr + 1) // 2, Nc // 2
                x = _plane((B, Nr, Nc), 8300)
                outs = [_nan((B, r2, c2)) for _ in range(4)]
                rc = L.emu_dwt2_fwd_wave(P(x), B, Nr, Nc, P(dlo), P(dhi), hlen, seg, guard, *[P(o) for o in outs])
                if rc == -2:
                    declined.add((0, hlen, seg))
                else:
                    assert rc == 0, (wname, guard, Nr, Nc, seg, rc)
                    cases.append(([0, B, Nr, Nc, hlen, seg, guard], [], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
                bands = [_plane((B, r2, c2), 8310 + k, signed=True) for k in range(4)]
                rec = _nan((B, Nr, Nc))
                rc = L.emu_dwt2_inv_wave(*[P(b) for b in bands], B, r2, c2, Nr, Nc, P(rlo), P(rhi), hlen, seg, guard, P(rec))
                if rc == -2:
                    declined.add((1, hlen, seg))
                else:
                    assert rc == 0, (wname, guard, Nr, Nc, seg, rc)
                    cases.append(([1, B, r2, c2, Nr, Nc, hlen, seg, guard], [], [(b, IN) for b in bands] + [(rlo, IN), (rhi, IN), (rec, OUT)]))
    assert any(c[0][0] == 0 and c[0][-1] == 0 for c in cases) and any(c[0][0] == 1 and c[0][-1] == 0 for c in cases)  # guard = 0 ran
    assert declined == WAVE_DECLINED and 2 * (total - len(cases)) <= total
    _run(programs("wave"), tmp_path, cases)



def test_dwt2_wave_two_levels_forward_under_sanitizers(programs, tmp_path):
    """dwt2_fwd2_wave: 16, 32, 240, 256 and 272 columns (a strip is 240: one strip to the column, one group into the second), 4, 8
    and 20 rows (second levels of one row: shorter than every filter but haar), one, two and all second-level rows per segment,
    2 ... 8 taps, one and two images, every one of the seven planes its own block.  Nothing is declined."""
    L = lib()
    cases = []
    for wname in WAVE_WNAMES:
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for N0c in (16, 32, 240, 256, 272):
            for N0r in (4, 8, 20):
                for seg2 in sorted({1, 2, N0r // 4}):
                    for B in (1, 2):
                        s1, s2 = [B * (N0r // 2) * (N0c // 2)] * 3, [B * (N0r // 4) * (N0c // 4)] * 4
                        x = _plane((B, N0r, N0c), 8400)
                        det1, band2 = _nan(sum(s1)), _nan(sum(s2))
                        assert L.emu_dwt2_fwd2_wave(P(x), B, N0r, N0c, P(dlo), P(dhi), hlen, seg2, P(det1), P(band2)) == 0
                        cases.append(([2, B, N0r, N0c, hlen, seg2], [], [(x, IN), (dlo, IN), (dhi, IN)] +
                                      [(p, OUT) for p in _split(det1, s1) + _split(band2, s2)]))
    _run(programs("wave"), tmp_path, cases)


# ----------------------------------------------------------------------------- register ring
def test_dwt2_ring_level_kernels_under_sanitizers(programs, tmp_path):
    """dwt2_ring_kernels.hpp, forward and inverse: 10, 16 and 20 taps, two and four columns per lane, 4, 8, 124, 128, 132 and 260
    columns (planes narrower than the filter; a strip of 128 or 256 columns to the column, one group short of it and one group into
    the next), 5, 33 and 34 rows, segments of 1 and 3 output rows and one whole walk, one and two images, the wavefront's LDS row
    sized to the element.  Nothing is declined."""
    L = lib()
    cases = []
    for wname in ("db5", "sym8", "db10"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for cpl in (2, 4):
            for Nc in (4, 8, 124, 128, 132, 260):
                for Nr in (5, 33, 34):
                    r2, c2 = (Nr + 1) // 2, Nc // 2
                    for seg in (1, 3, r2):
                        B = 1 + (Nc // 4 + Nr + seg) % 2
                        x = _plane((B, Nr, Nc), 8500)
                        outs = [_nan((B, r2, c2)) for _ in range(4)]
                        assert L.emu_dwt2_fwd_ring(P(x), B, Nr, Nc, P(dlo), P(dhi), hlen, seg, cpl, *[P(o) for o in outs]) == 0
                        cases.append(([0, B, Nr, Nc, hlen, seg, cpl], [], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
                        bands = [_plane((B, r2, c2), 8510 + k, signed=True) for k in range(4)]
                        rec = _nan((B, Nr, Nc))
                        assert L.emu_dwt2_inv_ring(*[P(b) for b in bands], B, r2, c2, Nr, Nc, P(rlo), P(rhi), hlen, seg, cpl, P(rec)) == 0
                        cases.append(([1, B, r2, c2, Nr, Nc, hlen, seg, cpl], [], [(b, IN) for b in bands] + [(rlo, IN), (rhi, IN), (rec, OUT)]))
    assert {c[0][1] for c in cases} == {1, 2}
    _run(programs("ring"), tmp_path, cases)


# ----------------------------------------------------------------------------- 1D in registers
def test_dwt1_in_registers_under_sanitizers(programs, tmp_path):
    """dwt1_reg_kernels.hpp, forward and inverse: rows of 2048, 2064 and 4112 samples (the shortest row, one 16-sample unit more, a
    second block of one unit), one to three levels, 2, 8 and 20 taps, one and three blocks per wavefront, one and three rows, every
    detail level its own block.  Nothing is declined."""
    L = lib()
    cases = []
    for wname in ("haar", "db4", "db10"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for N0 in (2048, 2064, 4112):
            for K in (1, 2, 3):
                for bpw in (1, 3):
                    for rows in (1, 3):
                        sizes = [rows * (N0 >> k) for k in range(1, K + 1)]
                        x = _plane((rows, N0), 8600)
                        det, app = _nan(sum(sizes)), _nan((rows, N0 >> K))
                        assert L.emu_dwt1_fwd_reg(P(x), rows, N0, K, P(dlo), P(dhi), hlen, bpw, P(det), P(app)) == 0
                        cases.append(([0, rows, N0, K, hlen, bpw], [], [(x, IN), (dlo, IN), (dhi, IN), (app, OUT)] + [(p, OUT) for p in _split(det, sizes)]))
                        det_in, app_in = _plane((sum(sizes),), 8610 + K, signed=True), _plane((rows, N0 >> K), 8620 + K, signed=True)
                        out = _nan((rows, N0))
                        assert L.emu_dwt1_inv_reg(P(app_in), P(det_in), rows, N0, K, P(rlo), P(rhi), hlen, bpw, P(out)) == 0
                        cases.append(([1, rows, N0, K, hlen, bpw], [], [(app_in, IN), (rlo, IN), (rhi, IN), (out, OUT)] + [(p, IN) for p in _split(det_in, sizes)]))
    _run(programs("reg1"), tmp_path, cases)


# ----------------------------------------------------------------------------- any-length stream kernels, a-trous row kernels
def _random_bank(hlen, seed):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.standard_normal(hlen), dtype=np.float32) for _ in range(4)]


def test_swt2_stream_level_under_sanitizers(programs, tmp_path):
    """swt_stream_kernels.hpp through emu_swt2_stream, forward and inverse: 10, 21 (a random bank: odd lengths are taken) and 40
    taps, dilations 1, 2 and 4, R = 2, 4 and 8 outputs per work item, odd and even rows (single columns / pairs), planes shorter
    than the filter on both axes, one and two images, the inverse with and without the soft threshold; the two planes between the
    launches are separate exact-size blocks.  Declined: dilation 4 on the planes of 4 rows (a dilation must be below both sizes)."""
    L = lib()
    cases, declined, total = [], set(), 0
    for hlen, bank in ((10, oracle.filters("db5")[1:]), (21, _random_bank(21, 21)), (40, oracle.filters("db20")[1:])):
        dlo, dhi, rlo, rhi = bank
        for Nr, Nc in ((4, 7), (4, 10), (5, 6), (9, 17), (12, 18), (33, 40)):
            for level in (1, 2, 3):
                for R in (2, 4, 8):
                    for B in (1, 2):
                        total += 3
                        x = _plane((B, Nr, Nc), 8700)
                        outs = [_nan((B, Nr, Nc)) for _ in range(4)]
                        rc = L.emu_swt2_stream(0, P(x), B, Nr, Nc, level, P(dlo), P(dhi), hlen, C.c_float(0.0), *[P(o) for o in outs], R)
                        if rc == -2:
                            declined.add((Nr, Nc, level))
                            continue
                        assert rc == 0, (hlen, Nr, Nc, level, R, rc)
                        cases.append(([0, 0, B, Nr, Nc, level, hlen, R], [0.0], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
                        bands = [_plane((B, Nr, Nc), 8710 + k, signed=True) for k in range(4)]
                        for beta in (0.0, 0.25):
                            rec = _nan((B, Nr, Nc))
                            assert L.emu_swt2_stream(1, P(rec), B, Nr, Nc, level, P(rlo), P(rhi), hlen, C.c_float(beta), *[P(b) for b in bands], R) == 0
                            cases.append(([0, 1, B, Nr, Nc, level, hlen, R], [beta], [(rec, OUT), (rlo, IN), (rhi, IN)] + [(b, IN) for b in bands]))
    assert declined == {(4, 7, 3), (4, 10, 3)} and 2 * (total - len(cases)) <= total
    _run(programs("stream"), tmp_path, cases)


def test_dwt2_stream_level_under_sanitizers(programs, tmp_path):
    """dwt2_stream_kernels.hpp through emu_dwt2_stream, forward and inverse: 10 and 40 taps, R = 2 and 4, half rows of odd and of even
    length (single columns / pairs in the column pass), planes shorter than the filter on both axes, one and two images; the two
    half-width planes between the launches are separate exact-size blocks.  Declined: 21 taps (even lengths only) and the plane of 7
    columns (even sizes only)."""
    L = lib()
    cases, declined, total = [], set(), 0
    for hlen, bank in ((10, oracle.filters("db5")[1:]), (21, _random_bank(21, 22)), (40, oracle.filters("db20")[1:])):
        dlo, dhi, rlo, rhi = bank
        for Nr, Nc in ((6, 10), (10, 12), (34, 36), (64, 70), (8, 7)):
            for R in (2, 4):
                for B in (1, 2):
                    total += 2
                    half = (B, Nr // 2, Nc // 2)
                    x = _plane((B, Nr, Nc), 8800)
                    outs = [_nan(half) for _ in range(4)]
                    rc = L.emu_dwt2_stream(0, P(x), B, Nr, Nc, P(dlo), P(dhi), hlen, R, *[P(o) for o in outs])
                    assert rc == (-2 if hlen & 1 or Nc & 1 else 0), (hlen, Nr, Nc, R, rc)
                    if rc == -2:
                        declined.add((hlen & 1, Nc & 1))
                        continue
                    cases.append(([1, 0, B, Nr, Nc, hlen, R], [], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
                    bands = [_plane(half, 8810 + k, signed=True) for k in range(4)]
                    rec = _nan((B, Nr, Nc))
                    assert L.emu_dwt2_stream(1, P(rec), B, Nr, Nc, P(rlo), P(rhi), hlen, R, *[P(b) for b in bands]) == 0
                    cases.append(([1, 1, B, Nr, Nc, hlen, R], [], [(rec, OUT), (rlo, IN), (rhi, IN)] + [(b, IN) for b in bands]))
    assert declined == {(1, 0), (1, 1), (0, 1)} and 2 * (total - len(cases)) <= total
    _run(programs("stream"), tmp_path, cases)


def test_swt1_split_rows_under_sanitizers(programs, tmp_path):
    """swt_split_kernels.hpp through emu_swt1_split, analysis and synthesis of rows: 16 ... 36 columns in steps of 4 (rows shorter than
    20 taps at every dilation), levels 1 ... 4 -- dilations 1, 2 and 4 through the LDS row kernels, their LDS what the launcher asks
    for; dilation 8 through the fwd4 / inv4p register kernels --, 4, 10 and 20 taps, one and three rows.  Nothing is declined."""
    L = lib()
    cases = []
    for wname in ("db2", "db5", "db10"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for Nc in range(16, 37, 4):
            for level in (1, 2, 3, 4):
                for Nr in (1, 3):
                    x, y = _plane((Nr, Nc), 8900), _plane((Nr, Nc), 8901, signed=True)
                    o0, o1 = _nan((Nr, Nc)), _nan((Nr, Nc))
                    assert L.emu_swt1_split(0, P(x), None, Nr, Nc, level, P(dlo), P(dhi), hlen, P(o0), P(o1)) == 0
                    cases.append(([0, Nr, Nc, level, hlen], [], [(x, IN), (None, IN), (dlo, IN), (dhi, IN), (o0, OUT), (o1, OUT)]))
                    r0 = _nan((Nr, Nc))
                    assert L.emu_swt1_split(1, P(x), P(y), Nr, Nc, level, P(rlo), P(rhi), hlen, P(r0), None) == 0
                    cases.append(([1, Nr, Nc, level, hlen], [], [(x, IN), (y, IN), (rlo, IN), (rhi, IN), (r0, OUT), (None, OUT)]))
    assert len(cases) == 3 * 6 * 4 * 2 * 2
    _run(programs("rows"), tmp_path, cases)
