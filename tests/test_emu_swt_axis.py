"""The depth-axis a-trous kernels of a stationary volume (pypwt_amd/csrc/swt3_axis_kernels.hpp) on the host against the numpy formula.

tests/cpu_emu/emu_swt_axis.cpp is compiled here with g++ -DPDWT_CPU_EMU (fp32, and fp64 with -DPDWT_DOUBLE): the kernels' tile
functions -- orbit and segment of a workgroup, first source slice by a true modulo, the wrapping counters, the register window
that shifts by one slot per step -- run workgroup by workgroup over the launcher's grid.  The reference is the formula itself in
fp64, as a matrix over the depth axis:

    forward   lo[g] = sum_j in[(g + (j - c) f) mod Nz] * dec_lo[hlen - 1 - j],  c = hlen / 2 - 1      (hi likewise)
    inverse   out[g] = 1/2 sum_j (lo[(g + (j - c) f) mod Nz] * rec_lo[hlen - 1 - j] + hi[same] * rec_hi[hlen - 1 - j]),  c = hlen / 2

(tests/test_volume_swt_ref_cpu.py pins the same formulas to pywt.swtn / pywt.iswtn.)

Swept: every even length from 2 to 40 taps -- the six built-in names of tests/test_emu_axis.py and the banks of tests/tap_banks.py,
in which no tap is below 0.079 --, fp32 and fp64, both directions, f in {1, 2, 4, 8, 16}, Nz from 1 to 41 (Nz < f, Nz no multiple
of f, Nz below hlen * f: the source counter wraps many times per window), the plane sizes PLANES of tests/test_emu_axis.py at both
access widths, segments of 1 and 2 steps and the chooser's for 1, 16 and 2048 resident workgroups.  Outputs are pre-filled with
NaN, so a slice the walk never wrote shows.

A thread's walk along the depth axis does not depend on the plane size, and the plane size decides nothing but the access width
and the last column group.  So the sweep has two parts, and every value above is in both:
  * the walk: every (length, type, direction, f, Nz from 1 to 41, width, segment choice) on planes of 1 to 5 samples (4: whole 16-B
    groups, the wide access of every instantiation);
  * the planes: every (length, type, direction, f, plane size of PLANES, width, segment choice) at the depths DEPTHS -- one slice,
    below every dilation but 1 and 2, odd, a power of two, and the largest;
and a third part runs a strided subset of what the two leave out of the full product, in case that argument misses something:
  * mid depths on large planes: every fourth Nz from 2 to 38 (and 41) on planes of 1024 samples (whole 16-B groups: both widths) and
    1025 (a dword per lane, five column groups, the last with one column), every length, type, direction, f and segment choice.

Bound: an output is a sum of at most 2 hlen products, so |error| <= 2 * hlen * eps * sum|taps| * max|x|.

The same source builds a stand-alone program under -fsanitize=address,undefined whose buffers are heap blocks of exactly the
input's and output's size, and whose outputs equal the plain build's bit for bit; nothing sanitised is loaded into python.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from test_emu_axis import BASE, CASES, LENGTHS, PLANES, SLOTS, filters_of

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_swt_axis.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("swt3_axis_kernels.hpp", "axis_common.hpp", "kernels_common.hpp", "strip_walk.hpp")]
DILATIONS = (1, 2, 4, 8, 16)
SMALL_PLANES = (1, 2, 3, 4, 5)
DEPTHS = (1, 3, 7, 16, 41)
MID_DEPTHS = tuple(range(2, 42, 4)) + (41,)
MID_PLANES = (1024, 1025)
_libs = {}


def emu(dtype):
    key = np.dtype(dtype).name
    if key in _libs:
        return _libs[key]
    so = os.path.join(HERE, "cpu_emu", "libpdwt_emu_swt_axis_%s.so" % ("f64" if dtype == np.float64 else "f32"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(BASE + ["-shared"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", so, SRC])
    lib = C.CDLL(so)
    lib.emu_swt_axis_width.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.emu_swt_axis_orbits.argtypes = [C.c_int, C.c_int]
    lib.emu_swt_axis_steps.argtypes = [C.c_int, C.c_int]
    lib.emu_swt_axis_seg.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int]
    lib.emu_swt_axis_cover.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.emu_swt_axis_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int]
    _libs[key] = lib
    return lib


def variants(lib, Nz, f, P, hlen, inverse):
    """(seg, width) of every launch shape: both access widths, every segment length the chooser returns, and 1 and 2 forced (a
    segment longer than the walk is one segment per orbit)."""
    out = []
    steps = lib.emu_swt_axis_steps(Nz, f)
    for width in sorted({1, lib.emu_swt_axis_width(P, hlen, inverse)}):
        chosen = {lib.emu_swt_axis_seg(Nz, f, P, hlen, width, s) for s in SLOTS}
        assert all(1 <= s <= steps for s in chosen), (chosen, steps)
        out += [(s, width) for s in sorted({1, 2} | chosen)]
    return out


def run(lib, x, Nz, P, f, hlen, lo, hi, seg, width, inverse):
    out = np.full((Nz if inverse else 2 * Nz, P), np.nan, dtype=x.dtype)
    rc = lib.emu_swt_axis_run(x.ctypes.data, out.ctypes.data, Nz, P, f, hlen, lo.ctypes.data, hi.ctypes.data, seg, width, int(inverse))
    assert rc == 0, (Nz, P, f, hlen, seg, width, inverse)
    return out


def operator(Nz, f, lo, hi, inverse):
    """The formula as a matrix in fp64 with the taps as the kernel got them: [2 Nz][Nz] forward, [Nz][2 Nz] inverse."""
    hlen = len(lo)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    c = hlen // 2 if inverse else hlen // 2 - 1
    M = np.zeros((Nz, 2 * Nz) if inverse else (2 * Nz, Nz))
    for g in range(Nz):
        for j in range(hlen):
            s = (g + (j - c) * f) % Nz
            if inverse:
                M[g, s] += 0.5 * lo[hlen - 1 - j]
                M[g, Nz + s] += 0.5 * hi[hlen - 1 - j]
            else:
                M[g, s] += lo[hlen - 1 - j]
                M[Nz + g, s] += hi[hlen - 1 - j]
    return M


def sweep(dtype, case, planes, depths):
    lib = emu(dtype)
    eps = float(np.finfo(dtype).eps)
    filt = filters_of(case, dtype)
    hlen, dlo, dhi, rlo, rhi = filt
    if not isinstance(case, str):
        assert min(float(np.abs(t).min()) for t in filt[1:]) >= 0.079  # every tap counts
    rng = np.random.default_rng(200 + hlen)
    pmax = max(planes)
    shapes = 0
    for inverse in (False, True):
        lo, hi = (rlo, rhi) if inverse else (dlo, dhi)
        taps = max(float(np.abs(lo).sum()), float(np.abs(hi).sum()))
        for Nz in depths:
            xall = (rng.standard_normal((2 * Nz if inverse else Nz, pmax)) * 100).astype(dtype)
            tol = 2 * hlen * eps * taps * float(np.abs(xall).max())
            for f in DILATIONS:
                wall = operator(Nz, f, lo, hi, inverse) @ xall.astype(np.float64)  # columns are independent: one product serves every P
                for P in planes:
                    x, want = np.ascontiguousarray(xall[:, :P]), wall[:, :P]
                    for seg, width in variants(lib, Nz, f, P, hlen, inverse):
                        got = run(lib, x, Nz, P, f, hlen, lo, hi, seg, width, inverse)
                        err = np.abs(got.astype(np.float64) - want).max()  # NaN: an output the walk never wrote
                        assert err <= tol, (Nz, P, f, hlen, seg, width, inverse, err, tol)
                        shapes += 1
    return shapes


IDS = [str(oracle.filters(c)[0]) if isinstance(c, str) else "bank%d" % c for c in CASES]


def test_every_even_length_is_built_and_no_other():
    lib = emu(np.float32)
    x = np.zeros((4, 4), dtype=np.float32)
    taps = np.zeros(64, dtype=np.float32)
    for hlen in range(0, 45):
        for inverse in (0, 1):
            out = np.zeros((4, 4), dtype=np.float32)
            rc = lib.emu_swt_axis_run(x.ctypes.data, out.ctypes.data, 2, 4, 1, hlen, taps.ctypes.data, taps.ctypes.data, 1, 1, inverse)
            assert (rc == 0) == (hlen in LENGTHS), hlen
    assert sorted({oracle.filters(c)[0] if isinstance(c, str) else c for c in CASES}) == list(LENGTHS)


def test_the_wide_access_fits_the_register_window():
    """16 B per lane while the window (HLEN slices forward, 2 HLEN inverse) is at most 16 x 16 B; never below one column."""
    for dtype, full in ((np.float32, 4), (np.float64, 2)):
        lib = emu(dtype)
        for hlen in LENGTHS:
            assert lib.emu_swt_axis_width(1024, hlen, 0) == max(full // (2 if hlen > 16 else 1), 1)
            assert lib.emu_swt_axis_width(1024, hlen, 1) == max(full // (4 if hlen > 16 else 2 if hlen > 8 else 1), 1)
            assert lib.emu_swt_axis_width(1023, hlen, 0) == lib.emu_swt_axis_width(1023, hlen, 1) == 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_walk_equals_the_formula_at_every_depth_and_dilation(dtype, case):
    shapes = sweep(dtype, case, SMALL_PLANES, range(1, 42))
    assert shapes >= 2 * 41 * len(DILATIONS) * len(SMALL_PLANES) * 2  # (at least segments of 1 and 2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_plane_size_at_both_widths(dtype, case):
    shapes = sweep(dtype, case, PLANES, DEPTHS)
    assert shapes >= 2 * len(DEPTHS) * len(DILATIONS) * len(PLANES) * 2  # (at least segments of 1 and 2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mid_depths_on_large_planes(dtype, case):
    shapes = sweep(dtype, case, MID_PLANES, MID_DEPTHS)
    assert shapes >= 2 * len(MID_DEPTHS) * len(DILATIONS) * len(MID_PLANES) * 2  # (at least segments of 1 and 2)


def test_orbits_and_segments_cover_every_output_slice_once():
    """gcd(f, Nz) orbits of Nz / gcd steps; for every segment length -- forced, the chooser's from one slot to many -- the segments of
    all orbits visit every output slice exactly once."""
    lib = emu(np.float32)
    buf = (C.c_int * 64)()
    for Nz in range(1, 42):
        for f in DILATIONS + (3, 6, 41, 82):
            orbits, steps = lib.emu_swt_axis_orbits(Nz, f), lib.emu_swt_axis_steps(Nz, f)
            assert orbits == math.gcd(f, Nz) and orbits * steps == Nz
            segs = {1, 2, 3, steps}
            for hlen in LENGTHS:
                for P in PLANES:
                    for slots in SLOTS + (0, 7, 100000):
                        seg = lib.emu_swt_axis_seg(Nz, f, P, hlen, 1, slots)
                        assert 1 <= seg <= steps
                        segs.add(seg)
            for seg in sorted(segs):
                n = lib.emu_swt_axis_cover(Nz, f, seg, buf, 64)
                assert n == Nz and sorted(buf[:n]) == list(range(Nz)), (Nz, f, seg, list(buf[:n]))
    # a big plane and few slices: one segment per orbit; tiny planes and many slices: the orbits are cut
    assert lib.emu_swt_axis_seg(8, 1, 4096 * 4096, 8, 4, 2048) == 8
    assert lib.emu_swt_axis_seg(4096, 1, 64, 8, 4, 2048) < 64


def test_depth_kernels_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Heap blocks of exactly the input's and output's size: every residue of P mod 4, depths below, at and above the dilation and
    the filter length, both widths, segments of 1, 2 and the chooser's.  The outputs equal the unsanitised build's, bit for bit."""
    for dtype in (np.float32, np.float64):
        lib = emu(dtype)
        exe = str(tmp_path / ("emu_swt_axis_san_%s" % np.dtype(dtype).name))
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_SWT_AXIS_MAIN",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
               "-static-libubsan"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", exe, SRC]
        subprocess.check_call(cmd)
        rng = np.random.default_rng(11)
        data, res = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
        want = []
        with open(data, "wb") as fh:
            for hlen in LENGTHS:
                _, dlo, dhi, rlo, rhi = filters_of("haar" if hlen == 2 else hlen, dtype)
                for inverse in (0, 1):
                    lo, hi = (rlo, rhi) if inverse else (dlo, dhi)
                    for P in (1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 258):
                        for Nz, f in ((1, 1), (1, 4), (2, 1), (3, 2), (3, 16), (8, 4), (9, 2), (12, 8), (41, 1), (41, 16)):
                            x = rng.standard_normal((2 * Nz if inverse else Nz, P)).astype(dtype)
                            for seg, width in variants(lib, Nz, f, P, hlen, inverse):
                                fh.write(np.array([Nz, P, f, hlen, seg, width, inverse], dtype=np.int64).tobytes())
                                fh.write(np.ascontiguousarray(lo).tobytes() + np.ascontiguousarray(hi).tobytes() + x.tobytes())
                                want.append(run(lib, x, Nz, P, f, hlen, lo, hi, seg, width, inverse))
        r = subprocess.run([exe, data, res], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        assert int(r.stdout.split()[-1]) == len(want)
        got = np.fromfile(res, dtype=dtype)
        flat = np.concatenate([w.ravel() for w in want])
        assert got.shape == flat.shape and not np.isnan(flat).any()
        assert np.array_equal(got, flat)
