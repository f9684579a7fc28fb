"""tests/volume_spin_ref.py against what it must agree with, on the CPU: the roll convention is the 2D circshift's, one shift of
zero is the plain denoiser, and -- the identity that makes the feature meaningful -- the mean over all 2^3 shifts of a one-level
haar transform IS the stationary one-level haar denoiser.

The tolerance of tests/test_gpu_volume_spin.py is derived here from the reference alone: K_TOL = 4 times the distance between the
fp32 composition and the fp64-accumulated one, per case.  That it is tight enough is proved with the reference too: unshifting ONE
of the K reconstructions by one voxel too many, on any single axis, moves the mean by at least 100 such tolerances, for every case.
"""
import numpy as np
import pytest

import volume_ref
import volume_spin_ref as spin
import volume_swt_ref
from oracle import oracle


def test_the_roll_convention_is_the_2d_circshifts_slice_by_slice():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 7, 10)).astype(np.float32)
    for sr, sc in ((0, 0), (1, 0), (0, 3), (5, 9), (2, 4)):
        got = spin.shift(x, (0, sr, sc))
        for z in range(x.shape[0]):
            assert np.array_equal(got[z], oracle.circshift(x[z], sr, sc)), (sr, sc, z)
    # depth moves in the same sense: out[z] = in[z - sz]
    assert np.array_equal(spin.shift(x, (1, 0, 0))[1], x[0])
    assert np.array_equal(spin.shift(x, (-1, 0, 0))[0], x[1])
    assert np.array_equal(spin.shift(x, (-13, 27, -40)), spin.shift(x, (-13 % 4, 27 % 7, -40 % 10)))


def test_the_lattice_is_documented_and_has_no_repeats():
    lat = spin.lattice(64)
    assert lat[:8].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]
    assert lat[8].tolist() == [0, 0, 2] and len({tuple(p) for p in lat.tolist()}) == 64 and lat.max() == 3
    assert np.array_equal(spin.lattice(5), lat[:5])


@pytest.mark.parametrize("double", [False, True, "full"])
def test_one_shift_of_zero_is_the_plain_denoiser(double):
    x = np.random.default_rng(5).uniform(0, 255, size=(9, 10, 12)).astype(np.float32)
    L = volume_ref.clamp_levels(x.shape, volume_ref.hlen_of("db2"), 2)
    for mode, do_app in (("soft", 0), ("hard", 1)):
        got = spin.cycle_spin(x, "db2", 2, [(0, 0, 0)], mode, spin.BETA, do_app=do_app, double=double)
        bands = volume_ref.threshold(volume_ref.forward(x, "db2", L, double), L, mode, spin.BETA, do_app, 0)
        want = volume_ref.inverse(bands, x.shape, "db2", L, double)
        assert np.array_equal(got, want.astype(got.dtype)), (mode, do_app)


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_all_eight_shifts_of_one_haar_level_are_the_stationary_haar_denoiser(mode):
    x = np.random.default_rng(7).uniform(0, 255, size=(6, 8, 10))
    got, _, share = spin.cycle_spin(x, "haar", 1, spin.lattice(8), mode, spin.BETA, double="full", parts=True)
    assert 0.2 <= share <= 0.8, share
    bands = volume_swt_ref.threshold(volume_swt_ref.forward(x, "haar", 1, "full"), 1, mode, spin.BETA, 0, 0)
    want = volume_swt_ref.inverse(bands, "haar", 1, "full")
    err = float(np.abs(got - want).max())
    assert err <= 64 * 2.0 ** -52 * 255.0, err
    # ... and it is not the decimated denoiser
    assert float(np.abs(spin.cycle_spin(x, "haar", 1, [(0, 0, 0)], mode, spin.BETA, double="full") - want).max()) > 1.0


@pytest.mark.parametrize("case", spin.CASES, ids=spin.case_id)
def test_the_tolerance_tells_one_voxel_of_a_wrong_unshift(case):
    ref, tol = spin.tolerance(case)
    assert tol > 0
    mean, recs, share = spin.run_case(case, True, parts=True)
    assert np.array_equal(mean, ref)
    if case[5] is None:  # a global beta: chosen so that the operator neither keeps nor kills everything
        assert 0.2 <= share <= 0.8, share
    shifts = spin.lattice(8)
    worst = np.inf
    for k in range(len(recs)):
        for axis in range(3):
            wrong = shifts.copy()
            wrong[k, axis] += 1
            moved = float(np.abs(spin.mean_of(recs, wrong, True) - ref).max())
            worst = min(worst, moved / tol)
    print("volume-spin %s: tol %.3g (max |ref| %.3g), zeroed %.2f, one voxel off is at least %.0f tol" % (
        spin.case_id(case), tol, float(np.abs(ref).max()), share, worst))
    assert worst >= 100.0, worst
    # the fp64 bound of the GPU test, 1e-12 max |ref|, is further away still
    full = spin.run_case(case, "full", dtype=np.float64)
    assert 1e-12 * float(np.abs(full).max()) < tol


def test_the_adaptive_cases_have_no_zero_by_construction_in_the_noise_band():
    """The premise of volume_spin_ref.METHOD_SHAPES: the median that skips exact zeros is taken over the whole of ddd_1 in every
    shift of every adaptive case -- and it would not be on the odd haar shape, which is why that shape has no adaptive case."""
    for case in spin.CASES:
        if case[5] is None:
            continue
        shape, wname, levels = case[:3]
        x = spin.case_input(case)
        L = volume_ref.clamp_levels(shape, volume_ref.hlen_of(wname), levels)
        for s in spin.lattice(8):
            for double in (False, True):
                ddd1 = volume_ref.forward(spin.shift(x, s), wname, L, double)[7]
                assert float(np.abs(ddd1).min()) > 1e-3, (spin.case_id(case), s, double)
    x = np.random.default_rng(9).uniform(0, 255, size=(5, 7, 11)).astype(np.float32)
    assert int(np.count_nonzero(volume_ref.forward(x, "haar", 2, False)[7] == 0)) == 72 - 2 * 3 * 5
