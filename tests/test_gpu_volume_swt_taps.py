"""Tap-resolved GPU parity of the a-trous depth kernels of a stationary volume (pypwt_amd/csrc/swt3_axis_kernels.hpp): every even
filter length from 2 to 40 taps x every access width x both directions through `Wavelets3D(..., do_swt=1)`, at dilations 1, 2 and 4,
with the banks of tests/tap_banks.py -- four independent filters, no tap below 0.079 -- at the tolerance the reference itself sets.

tests/test_gpu_volume_swt.py runs the built-in Daubechies banks at 1.5e-6 (1 + L) max|ref|, which cannot see 14 of db20's 80 analysis
taps (tests/test_volume_swt_taps_cpu.py pins it), planes of whole 16-B groups only beyond 4 taps, and dilations above 1 with haar,
db2 and db4.  Each <HLEN, VEC, INV> is a template instantiation of its own: a register window of HLEN (the synthesis: 2 HLEN) slots
that shifts by one per step, the taps staged in LDS from 18 taps on, 16-B, 8-B and 4-B accesses, a by-value argument struct.
tests/test_emu_swt_axis.py proves the index math on the host; what gfx950 makes of each instantiation shows only here.

A volume is created with the built-in wavelet of n taps, its bank is replaced through the test hook pdwt_volume_set_filters (the depth
passes and every level's 2D step), and every band is compared with the per-axis composition with fp64 accumulation
(tests/volume_swt_ref.py, double=True) at K x the fp32 composition's own distance from it (tap_banks.volume_swt_forward_reference;
K = tap_banks.K), floored at one ulp.  The inverse is tested on its own: from the reference's fp32 bands (set_coeff), against the
f64acc composition's inverse.  tests/test_volume_swt_taps_cpu.py proves that zeroing any single tap of the depth steps alone is at
least 1000 tolerances away.

Level 1 (tap_banks.volume_shapes):  A = (n + 7, 8, 12): odd depth, one orbit of n + 7 steps, planes of 96 samples;
                                    B = (3 or 7, 9, 11): depth far below the filter (the source counter wraps many times per window),
                                        planes of 99 samples -- one column per lane in both directions.
Dilations above 1 (tap_banks.SWT_DILATED): the smallest volumes the level clamp lets reach them; (24, 25, 27) has 2 and 4 orbits.
The columns per thread of BOTH directions are asserted (depth_schedule; pdwt_volume_depth_width for the synthesis, which holds twice
the window): fp32 forward 4 up to 16 taps, then 2; inverse 4 up to 8 taps, 2 up to 16, then 1; fp64 forward 2 up to 16 taps, then 1;
inverse 2 up to 8 taps, then 1; one wherever a plane is not made of whole groups.  A case that lands on another width fails.
pdwt_volume_set_depth_segments forces segments of 1, 3 and 5 steps and one whole walk on A (B: the chooser's value and the whole
walk; the dilated cases: 1, 3 and the whole walk at every level, so blockIdx.y carries orbit x segment with both above 1); every
forced run gives the bits of the run at the chooser's value -- the arithmetic per output slice is the same.

fp64 (`Wavelets3D64`): the level-1 sweep and the (37, 36, 40) case, the bank cast to float64, against the fp64 composition ("full")
at the project's fp64 rule 1e-12 max(max|ref|, 1) per band; segments of 1 and 3 steps and the whole walk on A.

err / noise (fp32), err / bound (fp64) per (precision, n, shape, width, direction, segment) is recorded; test_report counts the
cases and prints the table (profiles/volume_swt_taps_parity.txt is the MI355X run's; PDWT_VOLUME_SWT_TAPS_PARITY_OUT=<file> writes it)."""
import os
from math import gcd

import numpy as np
import pytest

from oracle import oracle
import tap_banks
import volume_swt_ref

pytestmark = pytest.mark.gpu

LENGTHS = tuple(range(2, 41, 2))
SEGS_A32 = (1, 3, 5, "walk")
SEGS_A64 = (1, 3, "walk")
SEGS_B = ("chosen", "walk")
SEGS_DILATED = (1, 3, "walk")
DILATED64 = (1,)  # indices of tap_banks.SWT_DILATED that run in fp64 too: (37, 36, 40), 10 taps, two levels
RATIOS = {}  # (precision, n, shape label, width, direction, seg) -> err / noise (fp32), err / bound (fp64)


@pytest.fixture(scope="module")
def classes():
    oracle.build()
    from pypwt_amd import Wavelets3D, Wavelets3D64
    return {np.float32: Wavelets3D, np.float64: Wavelets3D64}


def widths_of(n, plane, dtype):
    """(forward, inverse) columns per thread: swt3_wide (swt3_axis_kernels.hpp) where the plane is made of whole groups, else 1."""
    full = 16 // np.dtype(dtype).itemsize
    fwd = max(full // (2 if n > 16 else 1), 1)
    inv = max(full // (4 if n > 16 else 2 if n > 8 else 1), 1)
    return tuple(w if plane % w == 0 else 1 for w in (fwd, inv))


def plan_of(cls, dtype, x, n, levels, filt):
    W = cls(x.astype(dtype), "db%d" % (n // 2), levels, do_swt=1)
    assert (W.levels, W.hlen, W.nbands, W.do_swt) == (levels, n, 1 + 7 * levels, 1)
    W._set_filters(filt)
    return W


def widths(W, n, shape, dtype):
    """The widths the volume reports at every level, asserted against the rule; returns level 1's (forward, inverse)."""
    want = widths_of(n, shape[1] * shape[2], dtype)
    for l in range(1, W.levels + 1):
        got = (W.depth_schedule(l)[0], W._depth_width(l, True))
        assert W._depth_width(l, False) == got[0]
        assert got == want, (n, shape, l, got, want)
    return want


def force(W, shape, seg):
    """Forces `seg` steps per segment at every level in both directions ("walk": one segment per orbit, "chosen": the chooser's)."""
    for l in range(1, W.levels + 1):
        steps = shape[0] // gcd(1 << (l - 1), shape[0])  # swt3_steps: the outputs of one orbit
        s = steps if seg == "walk" else 0 if seg == "chosen" else min(seg, steps)
        W._set_depth_segments(l, s, s)
        _, seg_fwd, seg_inv = W.depth_schedule(l)
        if seg != "chosen":
            assert (seg_fwd, seg_inv) == (s, s), (shape, l, seg, seg_fwd, seg_inv)
        assert 1 <= seg_fwd <= steps and 1 <= seg_inv <= steps


def note(prec, n, label, width, direction, seg, value):
    key = (prec, n, label, width, direction, str(seg))
    assert key not in RATIOS, key
    RATIOS[key] = value


def ratio(err, noise):
    return err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))


def run_both(W, x, coef):
    """(bands of the forward of x, image of the inverse alone from `coef`)"""
    W.set_image(x)
    W.forward()
    bands = [W.coeff_only(num) for num in range(W.nbands)]
    for num, c in enumerate(coef):
        W.set_coeff(c, num)
    W.inverse()
    return bands, W.image


def sweep32(W, x, n, label, segs, recorded, ref, tols, iref, itol, inoise, wf, wi):
    """Every segment length of `segs` in both directions against the reference; every run after the first gives the first's bits.
    Returns the number of comparisons recorded."""
    base, ran = None, 0
    for seg in segs:
        force(W, x.shape, seg)
        bands, img = run_both(W, x, ref)
        worst = 0.0
        for num, (g, r, (tol, noise)) in enumerate(zip(bands, ref, tols)):
            assert g.dtype == np.float32 and g.shape == r.shape
            err = float(np.abs(g.astype(np.float64) - r).max())
            worst = max(worst, ratio(err, noise))
            print("volume-swt-taps n=%2d %s seg=%s fwd band %d: err %.3g tol %.3g err/noise %.2f" % (n, label, seg, num, err, tol, ratio(err, noise)))
            assert err <= tol, (n, label, seg, "forward", num, err, tol, noise)
        err = float(np.abs(img.astype(np.float64) - iref).max())
        print("volume-swt-taps n=%2d %s seg=%s inv: err %.3g tol %.3g err/noise %.2f" % (n, label, seg, err, itol, ratio(err, inoise)))
        assert err <= itol, (n, label, seg, "inverse", err, itol, inoise)
        if base is None:
            base = (bands, img)
        else:
            for num, (g, b) in enumerate(zip(bands, base[0])):
                assert np.array_equal(g, b), (n, label, seg, "forward bits", num)
            assert np.array_equal(img, base[1]), (n, label, seg, "inverse bits")
        if seg in recorded:
            note("fp32", n, label, wf, "fwd", seg, worst)
            note("fp32", n, label, wi, "inv", seg, ratio(err, inoise))
            ran += 2
    return ran


def sweep64(W, x, n, label, segs, recorded, ref, iref, wf, wi):
    base, ran = None, 0
    for seg in segs:
        force(W, x.shape, seg)
        bands, img = run_both(W, x, ref)
        worst = 0.0
        for num, (g, r) in enumerate(zip(bands, ref)):
            assert g.dtype == np.float64 and g.shape == r.shape
            err, bound = float(np.abs(g - r).max()), 1e-12 * max(float(np.abs(r).max()), 1.0)
            worst = max(worst, err / bound)
            assert err <= bound, (n, label, seg, "forward", num, err, bound)
        err, bound = float(np.abs(img - iref).max()), 1e-12 * max(float(np.abs(iref).max()), 1.0)
        print("volume-swt-taps fp64 n=%2d %s seg=%s: fwd %.2g inv %.2g of the bound" % (n, label, seg, worst, err / bound))
        assert err <= bound, (n, label, seg, "inverse", err, bound)
        if base is None:
            base = (bands, img)
        else:
            assert all(np.array_equal(g, b) for g, b in zip(bands, base[0])) and np.array_equal(img, base[1]), (n, label, seg, "bits")
        if seg in recorded:
            note("fp64", n, label, wf, "fwd", seg, worst)
            note("fp64", n, label, wi, "inv", seg, err / bound)
            ran += 2
    return ran


def dilated_label(index):
    n, shape, levels = tap_banks.SWT_DILATED[index]
    return "%dx%dx%d-L%d" % (shape + (levels,))


DILATED_IDS = ["%d-%s" % (tap_banks.SWT_DILATED[i][0], dilated_label(i)) for i in range(len(tap_banks.SWT_DILATED))]


# ---------------------------------------------------------------------------------------------------------------- fp32

@pytest.mark.parametrize("n", LENGTHS)
def test_fp32_every_length_width_direction_and_segment(classes, n):
    filt = tap_banks.bank(n, 2000 + n)
    ran = 0
    for i, shape in enumerate(tap_banks.volume_shapes(n)):
        x = tap_banks.volume_input(shape, 4100 + 2 * n + i)
        ref, tols = tap_banks.volume_swt_forward_reference(x, 1, filt)
        iref, (itol, inoise) = tap_banks.volume_swt_inverse_reference(ref, 1, filt)
        W = plan_of(classes[np.float32], np.float32, x, n, 1, filt)
        assert [W.band_shape(k) for k in range(8)] == [r.shape for r in ref] == [shape] * 8
        wf, wi = widths(W, n, shape, np.float32)
        if i == 0:
            assert (wf, wi) == (4 if n <= 16 else 2, 4 if n <= 8 else 2 if n <= 16 else 1), (n, shape, wf, wi)
            ran += sweep32(W, x, n, "A", ("chosen",) + SEGS_A32, SEGS_A32, ref, tols, iref, itol, inoise, wf, wi)
        else:
            assert (wf, wi) == (1, 1), (n, shape, wf, wi)
            ran += sweep32(W, x, n, "B", SEGS_B, SEGS_B, ref, tols, iref, itol, inoise, wf, wi)
        W.cleanup()
    assert ran == (len(SEGS_A32) + len(SEGS_B)) * 2


@pytest.mark.parametrize("index", range(len(tap_banks.SWT_DILATED)), ids=DILATED_IDS)
def test_fp32_dilations_above_one_with_orbits_and_segments(classes, index):
    n, shape, levels = tap_banks.SWT_DILATED[index]
    filt, x = tap_banks.swt_dilated_input(index)
    ref, tols = tap_banks.volume_swt_forward_reference(x, levels, filt)
    iref, (itol, inoise) = tap_banks.volume_swt_inverse_reference(ref, levels, filt)
    W = plan_of(classes[np.float32], np.float32, x, n, levels, filt)
    wf, wi = widths(W, n, shape, np.float32)
    assert (wf, wi) == {0: (4, 4), 1: (4, 2), 2: (2, 1), 3: (1, 1)}[index], (n, shape, wf, wi)
    if index == 3:  # both factors of blockIdx.y above 1: 2 and 4 orbits of 12 and 6 steps, cut into segments of 1 and 3
        assert [gcd(1 << (l - 1), shape[0]) for l in (1, 2, 3)] == [1, 2, 4]
    ran = sweep32(W, x, n, dilated_label(index), ("chosen",) + SEGS_DILATED, SEGS_DILATED, ref, tols, iref, itol, inoise, wf, wi)
    assert ran == len(SEGS_DILATED) * 2
    W.cleanup()


def test_a_zeroed_depth_tap_misses_by_the_factor_the_reference_predicts(classes):
    """Non-vacuity on the device: n = 22, shape A, forward, tap 0 of dec_lo zeroed through pdwt_volume_set_filters and compared with
    the INTACT bank's reference.  The hook hands one bank to the depth pass and to the level's 2D step, so the device's result must
    be the composition with that tap zeroed on all three axes (at the tolerance: the hook reached every pass), and it must miss the
    intact reference by at least half the factor tests/test_volume_swt_taps_cpu.py computes for that tap zeroed in the depth step
    alone.  The bank is restored and the volume passes again."""
    n = 22
    filt = tap_banks.bank(n, 2000 + n)
    shape = tap_banks.volume_shapes(n)[0]
    x = tap_banks.volume_input(shape, 4100 + 2 * n)
    ref, tols = tap_banks.volume_swt_forward_reference(x, 1, filt)
    predicted = tap_banks.swt_depth_tap_factor(x, 1, filt, 1, 0, ref, tols)
    assert predicted >= 1000.0
    zeroed = tap_banks.without_tap(filt, 1, 0)
    zref, ztols = tap_banks.volume_swt_forward_reference(x, 1, zeroed)
    W = plan_of(classes[np.float32], np.float32, x, n, 1, zeroed)
    W.forward()
    got = [W.coeff_only(num).astype(np.float64) for num in range(8)]
    for num, (g, r, (tol, _)) in enumerate(zip(got, zref, ztols)):
        assert float(np.abs(g - r).max()) <= tol, ("the zeroed bank did not reach every pass", num)
    factor = max(float(np.abs(g - r).max()) / tol for g, r, (tol, _) in zip(got, ref, tols))
    print("volume-swt-taps n=22 tap 0 of dec_lo zeroed: misses by %.0f tolerances, the depth step alone predicts %.0f" % (factor, predicted))
    assert factor >= predicted / 2, (factor, predicted)
    W._set_filters(filt)
    W.forward()
    for num, (r, (tol, _)) in enumerate(zip(ref, tols)):
        assert float(np.abs(W.coeff_only(num).astype(np.float64) - r).max()) <= tol, ("restored bank", num)


def test_the_width_hook_answers_for_both_kinds_of_volume_and_refuses_what_it_must(classes):
    from pypwt_amd import _lib
    x = tap_banks.volume_input((24, 8, 12), 78)
    Ws = classes[np.float32](x, "db5", 2, do_swt=1)  # 10 taps: the synthesis on half the analysis' columns
    Wd = classes[np.float32](x, "db5", 2)
    assert Ws.levels == Wd.levels == 1
    assert (Ws._depth_width(1, False), Ws._depth_width(1, True)) == (4, 2) and Ws.depth_schedule(1)[0] == 4
    assert Wd._depth_width(1, False) == Wd._depth_width(1, True) == Wd.depth_schedule(1)[0]
    lib = Ws._lib
    for W in (Ws, Wd):
        for level in (0, 2, -1):
            for inverse in (0, 1):
                assert lib.pdwt_volume_depth_width(W._h, level, inverse) == _lib.ERR_ARG, (level, inverse)
        with pytest.raises(ValueError):
            W._depth_width(2, True)
    assert lib.pdwt_volume_depth_width(None, 1, 0) == _lib.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- fp64

def bank64(filt):
    return (filt[0],) + tuple(t.astype(np.float64) for t in filt[1:])


@pytest.mark.parametrize("n", LENGTHS)
def test_fp64_every_length_width_direction_and_segment(classes, n):
    filt = bank64(tap_banks.bank(n, 2000 + n))
    ran = 0
    for i, shape in enumerate(tap_banks.volume_shapes(n)):
        x = tap_banks.volume_input(shape, 4100 + 2 * n + i).astype(np.float64)
        ref = volume_swt_ref.forward(x, None, 1, "full", filt=filt)
        iref = volume_swt_ref.inverse(ref, None, 1, "full", filt=filt)
        W = plan_of(classes[np.float64], np.float64, x, n, 1, filt)
        wf, wi = widths(W, n, shape, np.float64)
        if i == 0:
            assert (wf, wi) == (2 if n <= 16 else 1, 2 if n <= 8 else 1), (n, shape, wf, wi)
            ran += sweep64(W, x, n, "A", ("chosen",) + SEGS_A64, SEGS_A64, ref, iref, wf, wi)
        else:
            assert (wf, wi) == (1, 1), (n, shape, wf, wi)
            ran += sweep64(W, x, n, "B", SEGS_B, SEGS_B, ref, iref, wf, wi)
        W.cleanup()
    assert ran == (len(SEGS_A64) + len(SEGS_B)) * 2


@pytest.mark.parametrize("index", DILATED64, ids=[DILATED_IDS[i] for i in DILATED64])
def test_fp64_dilation_two(classes, index):
    n, shape, levels = tap_banks.SWT_DILATED[index]
    filt32, x32 = tap_banks.swt_dilated_input(index)
    filt, x = bank64(filt32), x32.astype(np.float64)
    ref = volume_swt_ref.forward(x, None, levels, "full", filt=filt)
    iref = volume_swt_ref.inverse(ref, None, levels, "full", filt=filt)
    W = plan_of(classes[np.float64], np.float64, x, n, levels, filt)
    wf, wi = widths(W, n, shape, np.float64)
    assert (wf, wi) == (2, 1), (n, shape, wf, wi)
    assert sweep64(W, x, n, dilated_label(index), ("chosen",) + SEGS_DILATED, SEGS_DILATED, ref, iref, wf, wi) == len(SEGS_DILATED) * 2
    W.cleanup()


# -------------------------------------------------------------------------------------------------------------- report

def test_report():
    """Closes the module: every (n, shape, segment, direction) ran and was compared -- level 1: 20 x (4 + 2) x 2 in fp32,
    20 x (3 + 2) x 2 in fp64; the dilated cases: 4 x 3 x 2 in fp32, 1 x 3 x 2 in fp64 --, each at the width its instantiation must
    have; prints the table of profiles/volume_swt_taps_parity.txt."""
    f32 = {k: v for k, v in RATIOS.items() if k[0] == "fp32"}
    f64 = {k: v for k, v in RATIOS.items() if k[0] == "fp64"}
    one32 = {k: v for k, v in f32.items() if k[2] in ("A", "B")}
    one64 = {k: v for k, v in f64.items() if k[2] in ("A", "B")}
    assert len(one32) == len(LENGTHS) * (len(SEGS_A32) + len(SEGS_B)) * 2 == 240, len(one32)
    assert len(one64) == len(LENGTHS) * (len(SEGS_A64) + len(SEGS_B)) * 2 == 200, len(one64)
    assert len(f32) - len(one32) == len(tap_banks.SWT_DILATED) * len(SEGS_DILATED) * 2 == 24, len(f32)
    assert len(f64) - len(one64) == len(DILATED64) * len(SEGS_DILATED) * 2 == 6, len(f64)
    for n in LENGTHS:
        want32 = {("A", 4 if n <= 16 else 2, "fwd"), ("A", 4 if n <= 8 else 2 if n <= 16 else 1, "inv"), ("B", 1, "fwd"), ("B", 1, "inv")}
        want64 = {("A", 2 if n <= 16 else 1, "fwd"), ("A", 2 if n <= 8 else 1, "inv"), ("B", 1, "fwd"), ("B", 1, "inv")}
        assert {k[2:5] for k in one32 if k[1] == n} == want32, n
        assert {k[2:5] for k in one64 if k[1] == n} == want64, n
    assert {k[1:3] for k in f32 if k not in one32} == {(tap_banks.SWT_DILATED[i][0], dilated_label(i)) for i in range(len(tap_banks.SWT_DILATED))}
    assert all(np.isfinite(v) for v in RATIOS.values())
    lines = ["volume-swt-taps-parity  fp32: max err/noise over the bands (forward) or of the volume (inverse), K = %g (at most %g);"
             % (tap_banks.K, tap_banks.K_MAX),
             "volume-swt-taps-parity  fp64: err as a fraction of the bound 1e-12 max(max|ref|, 1).  seg = steps per depth segment;",
             "volume-swt-taps-parity  shape A = (n + 7, 8, 12), B = (3 if n < 8 else 7, 9, 11); DxRxC-Ll: l levels, dilations up to 2^(l-1)"]
    for prec, table in (("fp32", f32), ("fp64", f64)):
        rows = sorted({k[1:5] for k in table}, key=lambda r: (r[1] not in ("A", "B"), r[0], r[1], r[3]))
        for n, shape, width, direction in rows:
            cells = [(k[5], v) for k, v in table.items() if k[1:5] == (n, shape, width, direction)]
            cells.sort(key=lambda c: (not c[0].isdigit(), int(c[0]) if c[0].isdigit() else 0, c[0]))
            lines.append("volume-swt-taps-parity  %s n=%2d %s width=%d %s  " % (prec, n, shape, width, direction) +
                         "  ".join(("seg=%s %.2f" if prec == "fp32" else "seg=%s %.1e") % c for c in cells))
        lines.append(("volume-swt-taps-parity  %s largest: %.2f" if prec == "fp32" else "volume-swt-taps-parity  %s largest: %.1e") % (prec, max(table.values())))
    print("\n" + "\n".join(lines))
    if os.environ.get("PDWT_VOLUME_SWT_TAPS_PARITY_OUT"):  # how profiles/volume_swt_taps_parity.txt is made
        with open(os.environ["PDWT_VOLUME_SWT_TAPS_PARITY_OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")
