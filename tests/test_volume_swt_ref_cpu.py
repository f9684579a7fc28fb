"""tests/volume_swt_ref.py -- the per-axis composition every GPU test of the stationary volume is compared with -- pinned from
three sides, on the CPU:

  * to PyWavelets: pywt.swtn's bands and pywt.iswtn as a linear operator on random coefficients (tests/golden/volume_swt.npz,
    recorded by tests/golden/make_volume_swt_golden.py), at 1e-12 absolute.  The file keeps pywt's float64 results in fixed point,
    rounded to 2^-43 = 1.2e-13 at the most, so the composition itself has 8.8e-13 of that 1e-12, not all of it; the four specified
    cases have small-integer inputs, a fifth small one (c4) has real-valued data and coefficients;
  * to the committed oracle: its y and x steps alone on an image are the oracle's 2D SWT, three levels, both directions, 1e-12;
  * to itself: the round trip on odd sizes, which pywt refuses, to 1e-12.
  * its f64acc mode (double=True: fp32 data and taps, one rounding per axis step -- the reference of tests/tap_banks.py's stationary
    helpers) to the fp64 one, on the golden cases, at a bound counted from the roundings and the filters' L1 norms.

The last test is about the resolving power of tests/test_gpu_volume_swt.py: zeroing ANY single tap of any of the four filters in
the depth step alone moves the composition by at least 1000 x the tolerance the GPU module compares at (in the band it moves
most), so a depth kernel that drops, shifts or mis-stages one tap cannot pass -- the method of tests/test_volume_taps_cpu.py.
"""
import os

import numpy as np
import pytest

from oracle import oracle
import tap_banks
import volume_swt_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12


@pytest.fixture(scope="module", autouse=True)
def built():
    oracle.build()


def golden():
    """{case: (x, wname, levels, fwd bands, coef, inv)} as float64; the file keeps the float64 results in fixed point, 2^-q."""
    z = np.load(os.path.join(HERE, "golden", "volume_swt.npz"))
    q = 2.0 ** -int(z["q"])
    out = {}
    for c in z["cases"]:
        c = str(c)
        out[c] = (z[c + "_x"].astype(np.float64), str(z[c + "_wname"]), int(z[c + "_levels"]), z[c + "_fwd"].astype(np.float64) * q,
                  z[c + "_coef"].astype(np.float64), z[c + "_inv"].astype(np.float64) * q)
    return out


def test_the_golden_file_holds_the_cases_of_the_issue():
    g = golden()
    assert [(v[0].shape, v[1], v[2]) for v in g.values()][:4] == [((8, 8, 8), "haar", 3), ((8, 12, 16), "db2", 2), ((4, 8, 12), "db10", 1),
                                                                  ((6, 10, 4), "bior1.3", 1)]
    # and one more with real-valued data: the four above are small integers (exact in both programs, and they keep the file small)
    assert list(g)[4:] == ["c4"] and np.abs(g["c4"][0] - np.rint(g["c4"][0])).min() > 0 and np.abs(g["c4"][4] - np.rint(g["c4"][4])).min() > 0
    assert all(np.array_equal(g[c][0], np.rint(g[c][0])) for c in ("c0", "c1", "c2", "c3"))
    assert os.path.getsize(os.path.join(HERE, "golden", "volume_swt.npz")) < 300 * 1000
    for x, wname, levels, fwd, coef, inv in g.values():
        assert fwd.shape == coef.shape == (1 + 7 * levels,) + x.shape and inv.shape == x.shape
        assert ref.band_shapes(x.shape, levels) == [x.shape] * (1 + 7 * levels)


@pytest.mark.parametrize("case", ["c0", "c1", "c2", "c3", "c4"])
def test_forward_bands_equal_pywt_swtn(case):
    x, wname, levels, fwd, _, _ = golden()[case]
    got = ref.forward(x, wname, levels, "full")
    assert len(got) == 1 + 7 * levels
    for num, (g, w) in enumerate(zip(got, fwd)):
        err = float(np.abs(g - w).max())
        assert g.dtype == np.float64 and err <= TOL, (case, num, err)  # (the stored values are rounded to 2^-43 = 1.2e-13 at the most)
    sw = ref.to_swtn(got, levels)
    assert len(sw) == levels and sorted(sw[0]) == sorted(ref.KEYS + ("aaa",)) and all(sorted(d) == list(ref.KEYS) for d in sw[1:])
    assert sw[0]["aaa"] is got[0] and sw[-1]["ddd"] is got[ref.num_of(1, "ddd")]


@pytest.mark.parametrize("case", ["c0", "c1", "c2", "c3", "c4"])
def test_inverse_operator_equals_pywt_iswtn(case):
    x, wname, levels, _, coef, inv = golden()[case]
    got = ref.inverse(list(coef), wname, levels, "full")
    err = float(np.abs(got - inv).max())
    assert got.shape == x.shape and err <= TOL, (case, err)


@pytest.mark.parametrize("wname", ["haar", "db2", "db4", "sym4", "bior1.3", "db10"])
@pytest.mark.parametrize("shape", [(32, 40), (33, 27)])
def test_the_y_and_x_steps_alone_are_the_oracles_2d_swt(wname, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.standard_normal(shape) * 10.0
    levels = 3
    want = oracle.forward(img, wname, levels, ndim=2, do_swt=1, double="full")
    got = ref.forward_2d(img, wname, levels, "full")
    assert len(got) == len(want) == 1 + 3 * levels
    for num, (g, w) in enumerate(zip(got, want)):
        assert np.abs(g - np.asarray(w).reshape(shape)).max() <= TOL, (wname, shape, num)
    coef = [rng.standard_normal(shape) * 10.0 for _ in range(1 + 3 * levels)]
    back = oracle.inverse(coef, shape, wname, levels, ndim=2, do_swt=1, double="full")
    assert np.abs(ref.inverse_2d(coef, wname, levels, "full") - back).max() <= TOL, (wname, shape)


@pytest.mark.parametrize("wname,levels", [("haar", 2), ("db2", 1), ("db4", 2), ("bior1.3", 1), ("db20", 1)])
def test_round_trip_on_odd_sizes(wname, levels):
    """(5, 7, 9): pywt.swtn wants multiples of 2^levels; the periodic formulas do not care.  Perfect reconstruction needs no more
    than the filter bank's own identity, whatever the signal length (the depth of 5 is below every filter here but haar's)."""
    x = np.random.default_rng(579).uniform(0.0, 255.0, (5, 7, 9))
    bands = ref.forward(x, wname, levels, "full")
    assert all(b.shape == x.shape for b in bands)
    back = ref.inverse(bands, wname, levels, "full")
    assert np.abs(back - x).max() <= TOL * 255.0, (wname, float(np.abs(back - x).max()))


def test_fp32_mode_is_fp32_throughout_and_near_the_fp64_one():
    x = np.random.default_rng(3).uniform(0.0, 255.0, (6, 10, 12)).astype(np.float32)
    b32, b64 = ref.forward(x, "db2", 1, False), ref.forward(x, "db2", 1, "full")
    assert all(b.dtype == np.float32 for b in b32) and all(b.dtype == np.float64 for b in b64)
    assert max(float(np.abs(a - b).max()) for a, b in zip(b32, b64)) <= 1e-5 * 255.0 * 4
    assert ref.inverse(b32, "db2", 1, False).dtype == np.float32


U32 = 2.0 ** -24  # the relative error of one rounding to fp32


@pytest.mark.parametrize("case", ["c0", "c1", "c2", "c3", "c4"])
def test_f64acc_mode_is_one_rounding_per_axis_step_away_from_the_fp64_one(case):
    """double=True: fp32 data and taps, every axis step summed in fp64 and rounded to fp32 once.  Compared with "full" on the same
    fp32 input and the same fp32 taps (exact in fp64), so the roundings of the steps are all that differs.

    The bound.  N = the largest L1 norm of the two filters of a direction (the synthesis: (|rec_lo|_1 + |rec_hi|_1) / 2, its two
    half sums share one rounding), M = max |input|.  After s axis steps every exact value is at most N^s M; step s rounds a value of
    at most that size (error <= u N^s M, u = 2^-24) and carries the earlier error through a filter (factor N):
    e_s <= N e_(s-1) + u N^s M, so e_s <= s u N^s M.  L levels are s = 3 L steps; one more u N^s M covers what the recursion
    drops -- the fp64 sums' own error (hlen 2^-53 per step) and the growth (1 + u)^s of the rounded values: (3 L + 1) u N^(3 L) M."""
    x64, wname, levels, _, coef64, _ = golden()[case]
    x = x64.astype(np.float32)
    filt = tuple(oracle.filters(wname, np.float32))
    acc, full = ref.forward(x, None, levels, True, filt=filt), ref.forward(x, None, levels, "full", filt=filt)
    f32 = ref.forward(x, None, levels, False, filt=filt)
    l1 = [float(np.abs(np.asarray(t, dtype=np.float64)).sum()) for t in filt[1:5]]
    steps = 3 * levels
    bound = (steps + 1) * U32 * max(l1[0], l1[1]) ** steps * float(np.abs(x).max())
    worst = 0.0
    for num, (a, f) in enumerate(zip(acc, full)):
        assert a.dtype == np.float32 and f.dtype == np.float64 and a.shape == f.shape == x.shape
        worst = max(worst, float(np.abs(a.astype(np.float64) - f).max()))
        assert float(np.abs(a.astype(np.float64) - f).max()) <= bound, (case, num, bound)
    coef = [c.astype(np.float32) for c in coef64]
    iacc, ifull = ref.inverse(coef, None, levels, True, filt=filt), ref.inverse(coef, None, levels, "full", filt=filt)
    ibound = (steps + 1) * U32 * (0.5 * (l1[2] + l1[3])) ** steps * max(float(np.abs(c).max()) for c in coef)
    ierr = float(np.abs(iacc.astype(np.float64) - ifull).max())
    assert iacc.dtype == np.float32 and ierr <= ibound, (case, ierr, ibound)
    print("f64acc %s: forward %.3g of %.3g, inverse %.3g of %.3g" % (case, worst, bound, ierr, ibound))
    # ONE axis step is the fp64 step rounded, bit for bit (the same sums in the same order), and nothing of "full" or False moved
    lo, hi = ref.analysis_axis(x, filt[1], filt[2], 1, 0, True)
    wlo, whi = ref.analysis_axis(x.astype(np.float64), filt[1].astype(np.float64), filt[2].astype(np.float64), 1, 0)
    assert np.array_equal(lo, wlo.astype(np.float32)) and np.array_equal(hi, whi.astype(np.float32))
    back = ref.synthesis_axis(lo, hi, filt[3], filt[4], 1, 0, True)
    wide = ref.synthesis_axis(lo.astype(np.float64), hi.astype(np.float64), filt[3].astype(np.float64), filt[4].astype(np.float64), 1, 0)
    assert np.array_equal(back, wide.astype(np.float32))
    # the fp32 mode rounds every product and sum: where it differs from the fp64 one at all, it is no closer than the f64acc mode
    e32 = max(float(np.abs(a.astype(np.float64) - f).max()) for a, f in zip(f32, full))
    assert worst <= e32 or e32 == 0.0, (case, worst, e32)


def test_the_modes_are_full_true_and_false_and_nothing_else():
    x = np.zeros((2, 2, 2), dtype=np.float32)
    for bad in ("f64acc", 2, None, "True"):
        with pytest.raises(ValueError):
            ref.forward(x, "haar", 1, bad)


def test_thresholds_are_ops_refs_per_level():
    import ops_ref
    rng = np.random.default_rng(5)
    bands = [(rng.standard_normal((4, 4, 4)) * 20).astype(np.float32) for _ in range(15)]
    out = ref.threshold(bands, 2, "soft", 9.0, do_app=1, normalize=1)
    betas = ops_ref.level_betas(9.0, 2, 1, np.float32)
    assert ops_ref.same_bits(out[ref.num_of(2, "dad")], ops_ref.soft(bands[ref.num_of(2, "dad")], betas[1]))
    assert ops_ref.same_bits(out[0], ops_ref.soft(bands[0], ops_ref.app_beta(9.0, 2, 1, np.float32)))
    assert np.array_equal(ref.threshold(bands, 2, "hard", 9.0)[0], bands[0])


# ------------------------------------------------------------------------------------------------ one dropped depth tap
MIN_FACTOR = 1000.0


def gpu_tol32(ref64, ref32, levels):
    """tests/test_gpu_volume_swt.py's bound (tol32 of tests/test_gpu_volume.py)."""
    return max(1.5e-6 * (1 + levels) * max(float(np.abs(ref64).max()), 1.0), 2.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()))


def bank_of(case):
    return tuple(oracle.filters(case, np.float32)) if isinstance(case, str) else tap_banks.bank(case, 700 + case)


@pytest.mark.parametrize("case", ["haar", "db2", "db4", 6, 16, 18, 40], ids=str)
def test_a_single_dropped_depth_tap_is_1000_tolerances_away(case):
    """Built-in banks whose taps are all of ordinary size, and tap_banks banks (no tap below 0.079) for the long lengths, where the
    built-in wavelets' smallest taps are far below fp32's resolution (db20: 2e-10).  One level on (12, 10, 12) -- a depth below
    the long filters, P = 120 -- with the GPU module's data range and its tolerance."""
    filt = bank_of(case)
    n = filt[0]
    shape = (12, 10, 12)
    x = np.random.default_rng(1200 + n).uniform(0.0, 255.0, shape).astype(np.float32)
    f64 = ref.forward(x, None, 1, "full", filt=filt)
    f32 = ref.forward(x, None, 1, False, filt=filt)
    tols = [gpu_tol32(a, b, 1) for a, b in zip(f64, f32)]
    coef = [b.astype(np.float32) for b in f64]
    i64 = ref.inverse(coef, None, 1, "full", filt=filt)
    itol = gpu_tol32(i64, ref.inverse(coef, None, 1, False, filt=filt), 1)
    worst = np.inf
    for which in (1, 2):
        for j in range(n):
            got = ref.forward(x, None, 1, "full", filt=filt, depth_filt=tap_banks.without_tap(filt, which, j))
            factor = max(float(np.abs(g - r).max()) / t for g, r, t in zip(got, f64, tols))
            worst = min(worst, factor)
            assert factor >= MIN_FACTOR, (case, "forward", which, j, factor)
    for which in (3, 4):
        for j in range(n):
            got = ref.inverse(coef, None, 1, "full", filt=filt, depth_filt=tap_banks.without_tap(filt, which, j))
            factor = float(np.abs(got - i64).max()) / itol
            worst = min(worst, factor)
            assert factor >= MIN_FACTOR, (case, "inverse", which, j, factor)
    print("stationary volume, %s: smallest change / tolerance = %.0f" % (case, worst))
