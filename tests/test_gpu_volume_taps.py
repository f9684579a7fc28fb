"""Tap-resolved GPU parity of the depth-axis kernels of a volume (pypwt_amd/csrc/dwt3_axis_kernels.hpp): every even filter length from
4 to 40 taps x both access widths x both directions through `Wavelets3D`, with the banks of tests/tap_banks.py -- four independent
filters, no tap below 0.079 -- at the tolerance the reference itself sets.

tests/test_gpu_volume.py runs the built-in orthogonal wavelets at 1.5e-6 (1 + L) max|ref|, which cannot see 9 of db20's 40 taps
(tests/test_volume_taps_cpu.py pins it), and only 6 of the 20 lengths.  Each length is a template instantiation of its own with its
own register window; from 18 taps on the taps are staged in LDS and the wide access is halved; the parity of hlen / 2 chooses the
synthesis shift.  Here a volume is created with a built-in wavelet of n taps (one level), its bank is replaced through the test hook
pdwt_volume_set_filters (the depth passes and the level's 2D plan), and every band is compared with the one-level composition of the
oracle with fp64 accumulation (tests/volume_ref.py, double=True) at K x the fp32 composition's own distance from it
(tap_banks.volume_forward_reference; K = tap_banks.K), floored at one ulp.  The inverse is tested on its own: from the reference's
fp32 coefficients (set_coeff), against the f64acc composition's inverse.  tests/test_volume_taps_cpu.py proves that zeroing any
single tap of the depth step alone is at least 1000 tolerances away.

Shapes (tap_banks.volume_shapes):   A = (n + 7, 8, 12): odd depth >= n, planes of 96 samples -- 4 columns per lane up to 16 taps, 2 from 18;
                                    B = (3 or 7, 9, 11): depth below the filter length (the source counter wraps up to six times per
                                        window), planes of 99 samples -- one column per lane.
The width is asserted through depth_schedule; a case that lands on the other width fails.  The chooser gives one step per workgroup
at these sizes, so the second hook, pdwt_volume_set_depth_segments, forces segments of 1, 3 and 5 steps (several segments of several
steps and a ragged last one at every n) and one whole walk on shape A, in both directions; shape B runs at the chooser's value and
as one whole walk.  Nothing is excluded: 19 x (4 + 2) x 2 comparisons in fp32, counted by test_report.

fp64 (`Wavelets3D64`): the same lengths and shapes, the bank cast to float64, against the fp64 composition ("full") at the project's
fp64 rule 1e-12 max(max|ref|, 1) per band; segments of 1 and 3 steps and the whole walk on A.  Its wide path is 2 columns up to 16
taps and absent beyond.

err / noise per (n, shape, width, direction, segment) is recorded; test_report prints the table (profiles/volume_taps_parity.txt is the
MI355X run's; PDWT_VOLUME_TAPS_PARITY_OUT=<file> writes it)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle
import tap_banks
import volume_ref

pytestmark = pytest.mark.gpu

LENGTHS = tuple(range(4, 41, 2))
SEGS_A32 = (1, 3, 5, "walk")
SEGS_A64 = (1, 3, "walk")
SEGS_B = ("chosen", "walk")
RATIOS = {}  # (precision, n, shape "A" / "B", width, direction, seg) -> err / noise (fp32), err / bound (fp64)


@pytest.fixture(scope="module")
def classes():
    oracle.build()
    from pypwt_amd import Wavelets3D, Wavelets3D64
    return {np.float32: Wavelets3D, np.float64: Wavelets3D64}


def div2(n):
    return (n + (n & 1)) // 2


def steps_of(nz, n):
    """(forward, inverse) steps of a whole walk: dwt3_fwd_steps, dwt3_inv_steps (dwt3_axis_kernels.hpp)."""
    shift = 0 if (n // 2) & 1 else 1
    return div2(nz), (nz - 1 + shift) // 2 + 1


def wide_of(n, dtype):
    """dwt3_wide: 16 B per lane up to 16 taps, 8 B from 18 taps on."""
    return (16 // np.dtype(dtype).itemsize) // (2 if n > 16 else 1)


def plan_of(cls, dtype, x, n, filt):
    W = cls(x.astype(dtype), "db%d" % (n // 2), 1)
    assert (W.levels, W.hlen, W.nbands) == (1, n, 8)
    W._set_filters(filt)
    return W


def force(W, shape, n, seg):
    """Forces `seg` steps per segment in both directions (\"walk\": one segment of all steps, \"chosen\": the chooser's) and returns
    what depth_schedule reports."""
    fwd, inv = steps_of(shape[0], n)
    want = {"walk": (fwd, inv), "chosen": (0, 0)}.get(seg, (seg, seg))
    W._set_depth_segments(1, *want)
    width, seg_fwd, seg_inv = W.depth_schedule(1)
    if seg != "chosen":
        assert (seg_fwd, seg_inv) == want, (n, shape, seg, seg_fwd, seg_inv)
    assert 1 <= seg_fwd <= fwd and 1 <= seg_inv <= inv
    return width


def expected_width(shape, n, dtype):
    wide = wide_of(n, dtype)
    return wide if (shape[1] * shape[2]) % wide == 0 else 1


def note(prec, n, i, width, direction, seg, value):
    key = (prec, n, "AB"[i], width, direction, str(seg))
    assert key not in RATIOS, key
    RATIOS[key] = value


def ratio(err, noise):
    return err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))


# ---------------------------------------------------------------------------------------------------------------- fp32

@pytest.mark.parametrize("n", LENGTHS)
def test_fp32_every_length_width_direction_and_segment(classes, n):
    filt = tap_banks.bank(n, 2000 + n)
    ran = 0
    for i, shape in enumerate(tap_banks.volume_shapes(n)):
        x = tap_banks.volume_input(shape, 4100 + 2 * n + i)
        ref, tols = tap_banks.volume_forward_reference(x, filt)
        iref, (itol, inoise) = tap_banks.volume_inverse_reference(ref, shape, filt)
        W = plan_of(classes[np.float32], np.float32, x, n, filt)
        assert [W.band_shape(k) for k in range(8)] == [r.shape for r in ref]
        for seg in (SEGS_A32 if i == 0 else SEGS_B):
            width = force(W, shape, n, seg)
            assert width == expected_width(shape, n, np.float32) == ((4 if n <= 16 else 2) if i == 0 else 1), (n, shape, width)
            W.set_image(x)
            W.forward()
            worst = 0.0
            for num, (r, (tol, noise)) in enumerate(zip(ref, tols)):
                err = float(np.abs(W.coeff_only(num).astype(np.float64) - r).max())
                worst = max(worst, ratio(err, noise))
                print("volume-taps n=%2d %s seg=%s fwd band %d: err %.3g tol %.3g err/noise %.2f" % (n, shape, seg, num, err, tol, ratio(err, noise)))
                assert err <= tol, (n, shape, seg, "forward", num, err, tol, noise)
            note("fp32", n, i, width, "fwd", seg, worst)
            # the inverse on its own: the reference's fp32 coefficients
            for num, r in enumerate(ref):
                W.set_coeff(r, num)
            W.inverse()
            err = float(np.abs(W.image.astype(np.float64) - iref).max())
            print("volume-taps n=%2d %s seg=%s inv: err %.3g tol %.3g err/noise %.2f" % (n, shape, seg, err, itol, ratio(err, inoise)))
            assert err <= itol, (n, shape, seg, "inverse", err, itol, inoise)
            note("fp32", n, i, width, "inv", seg, ratio(err, inoise))
            ran += 2
        W.cleanup()
    assert ran == (len(SEGS_A32) + len(SEGS_B)) * 2


def test_a_zeroed_depth_tap_misses_by_the_factor_the_reference_predicts(classes):
    """Non-vacuity on the device: n = 22, shape A, forward, tap 0 of dec_lo zeroed through pdwt_volume_set_filters and compared with
    the FULL bank's reference.  The hook hands one bank to the depth pass and to the level's 2D plan, so the device's result must be
    the composition with that tap zeroed on all three axes (at the tolerance: the hook reached every pass), and its distance from the
    full bank's reference must be the factor tests/test_volume_taps_cpu.py computes for that tap (zeroed in the depth step), within a
    factor of two.  The bank is restored and the volume passes again."""
    n = 22
    filt = tap_banks.bank(n, 2000 + n)
    shape = tap_banks.volume_shapes(n)[0]
    x = tap_banks.volume_input(shape, 4100 + 2 * n)
    ref, tols = tap_banks.volume_forward_reference(x, filt)
    predicted = tap_banks.depth_tap_factor(x, filt, 1, 0, ref, tols)
    assert predicted >= 1000.0
    zeroed = tap_banks.without_tap(filt, 1, 0)
    zref, ztols = tap_banks.volume_forward_reference(x, zeroed)
    W = plan_of(classes[np.float32], np.float32, x, n, zeroed)
    W.forward()
    got = [W.coeff_only(num).astype(np.float64) for num in range(8)]
    for num, (g, r, (tol, _)) in enumerate(zip(got, zref, ztols)):
        assert float(np.abs(g - r).max()) <= tol, ("the zeroed bank did not reach every pass", num)
    factor = max(float(np.abs(g - r).max()) / tol for g, r, (tol, _) in zip(got, ref, tols))
    print("volume-taps n=22 tap 0 of dec_lo zeroed: misses by %.0f tolerances, the depth step alone predicts %.0f" % (factor, predicted))
    assert predicted / 2 <= factor <= predicted * 2, (factor, predicted)
    W._set_filters(filt)
    W.forward()
    for num, (r, (tol, _)) in enumerate(zip(ref, tols)):
        assert float(np.abs(W.coeff_only(num).astype(np.float64) - r).max()) <= tol, ("restored bank", num)


def test_the_two_hooks_refuse_what_they_must_and_change_nothing_then(classes):
    from pypwt_amd import _lib
    n, shape = 8, (15, 8, 12)
    x = tap_banks.volume_input(shape, 77)
    W = classes[np.float32](x, "db4", 1)
    lib, h = W._lib, W._h
    created = W.depth_schedule(1)
    fwd, inv = steps_of(shape[0], n)
    assert created[0] == 4 and 1 <= created[1] <= fwd and 1 <= created[2] <= inv
    W._set_depth_segments(1, 3, 5)
    assert W.depth_schedule(1) == (created[0], 3, 5)
    for bad in ((1, fwd + 1, 1), (1, 1, inv + 1), (1, -1, 1), (1, 1, -2), (0, 1, 1), (2, 1, 1)):
        assert lib.pdwt_volume_set_depth_segments(h, *bad) == _lib.ERR_ARG, bad
        assert W.depth_schedule(1) == (created[0], 3, 5), bad
    W._set_depth_segments(1, 0, 5)
    assert W.depth_schedule(1) == (created[0], created[1], 5)
    W._set_depth_segments(1, 0, 0)
    assert W.depth_schedule(1) == created
    # a foreign length, a null filter: PDWT_ERR_ARG and the built-in db4 is still what runs
    W.forward()
    before = [W.coeff_only(num) for num in range(8)]
    rp = C.POINTER(C.c_float)
    for m in (6, 10):
        taps = [C.cast(t.ctypes.data, rp) for t in tap_banks.bank(m, 5)[1:]]
        assert lib.pdwt_volume_set_filters(h, m, *taps) == _lib.ERR_ARG
    taps = [C.cast(t.ctypes.data, rp) for t in tap_banks.bank(n, 5)[1:]]
    assert lib.pdwt_volume_set_filters(h, n, taps[0], taps[1], taps[2], C.cast(None, rp)) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        W._set_filters(tap_banks.bank(6, 5))
    assert W.info()["hlen"] == n and W.depth_schedule(1) == created
    W.forward()
    assert all(np.array_equal(W.coeff_only(num), b) for num, b in enumerate(before))
    # a bank of the volume's own length: image, coefficients and state are left alone
    state = W.info()["state"]
    W._set_filters(tap_banks.bank(n, 5))
    assert W.info()["state"] == state and np.array_equal(W.image, x)
    assert all(np.array_equal(W.coeff_only(num), b) for num, b in enumerate(before))
    assert W.depth_schedule(1) == created


# ---------------------------------------------------------------------------------------------------------------- fp64

@pytest.mark.parametrize("n", LENGTHS)
def test_fp64_every_length_width_direction_and_segment(classes, n):
    filt32 = tap_banks.bank(n, 2000 + n)
    filt = (n,) + tuple(t.astype(np.float64) for t in filt32[1:])
    ran = 0
    for i, shape in enumerate(tap_banks.volume_shapes(n)):
        x = tap_banks.volume_input(shape, 4100 + 2 * n + i).astype(np.float64)
        ref = volume_ref.forward(x, None, 1, "full", filt=filt)
        iref = volume_ref.inverse(ref, shape, None, 1, "full", filt=filt)
        W = plan_of(classes[np.float64], np.float64, x, n, filt)
        for seg in (SEGS_A64 if i == 0 else SEGS_B):
            width = force(W, shape, n, seg)
            assert width == expected_width(shape, n, np.float64) == ((2 if n <= 16 else 1) if i == 0 else 1), (n, shape, width)
            W.set_image(x)
            W.forward()
            worst = 0.0
            for num, r in enumerate(ref):
                g = W.coeff_only(num)
                assert g.dtype == np.float64 and g.shape == r.shape
                err, bound = float(np.abs(g - r).max()), 1e-12 * max(float(np.abs(r).max()), 1.0)
                worst = max(worst, err / bound)
                assert err <= bound, (n, shape, seg, "forward", num, err, bound)
            note("fp64", n, i, width, "fwd", seg, worst)
            for num, r in enumerate(ref):
                W.set_coeff(r, num)
            W.inverse()
            err, bound = float(np.abs(W.image - iref).max()), 1e-12 * max(float(np.abs(iref).max()), 1.0)
            assert err <= bound, (n, shape, seg, "inverse", err, bound)
            note("fp64", n, i, width, "inv", seg, err / bound)
            ran += 2
        W.cleanup()
    assert ran == (len(SEGS_A64) + len(SEGS_B)) * 2


# -------------------------------------------------------------------------------------------------------------- report

def test_report():
    """Closes the module: every (n, shape, segment, direction) ran and was compared -- 19 x (4 + 2) x 2 in fp32, 19 x (3 + 2) x 2 in
    fp64 --, both widths at every length; prints the table of profiles/volume_taps_parity.txt."""
    f32 = {k: v for k, v in RATIOS.items() if k[0] == "fp32"}
    f64 = {k: v for k, v in RATIOS.items() if k[0] == "fp64"}
    assert len(f32) == len(LENGTHS) * (len(SEGS_A32) + len(SEGS_B)) * 2 == 228, len(f32)
    assert len(f64) == len(LENGTHS) * (len(SEGS_A64) + len(SEGS_B)) * 2 == 190, len(f64)
    for n in LENGTHS:
        assert {k[2:5] for k in f32 if k[1] == n} == {(s, w, d) for s, w in (("A", 4 if n <= 16 else 2), ("B", 1)) for d in ("fwd", "inv")}, n
        assert {k[2:5] for k in f64 if k[1] == n} == {(s, w, d) for s, w in (("A", 2 if n <= 16 else 1), ("B", 1)) for d in ("fwd", "inv")}, n
    lines = ["volume-taps-parity  fp32: max err/noise over the 8 bands (forward) or of the volume (inverse), K = %g (at most %g);"
             % (tap_banks.K, tap_banks.K_MAX),
             "volume-taps-parity  fp64: err as a fraction of the bound 1e-12 max(max|ref|, 1).  seg = steps per depth segment;",
             "volume-taps-parity  shape A = (n + 7, 8, 12), B = (3 if n < 8 else 7, 9, 11)"]
    for prec, table in (("fp32", f32), ("fp64", f64)):
        for n, shape, width, direction in sorted({k[1:5] for k in table}):
            cells = [(k[5], v) for k, v in table.items() if k[1:5] == (n, shape, width, direction)]
            cells.sort(key=lambda c: (not c[0].isdigit(), int(c[0]) if c[0].isdigit() else 0, c[0]))
            lines.append("volume-taps-parity  %s n=%2d %s width=%d %s  " % (prec, n, shape, width, direction) +
                         "  ".join(("seg=%s %.2f" if prec == "fp32" else "seg=%s %.1e") % c for c in cells))
        lines.append(("volume-taps-parity  %s largest: %.2f" if prec == "fp32" else "volume-taps-parity  %s largest: %.1e") % (prec, max(table.values())))
    print("\n" + "\n".join(lines))
    if os.environ.get("PDWT_VOLUME_TAPS_PARITY_OUT"):  # how profiles/volume_taps_parity.txt is made
        with open(os.environ["PDWT_VOLUME_TAPS_PARITY_OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")
