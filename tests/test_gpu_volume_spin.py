"""Circular shifts and cycle spinning of volumes on the GPU -- `circshift`, `set_cycle_spinning` / `last_shift`, `cycle_spin` and
`spin_footprint` of `Wavelets3D` / `Wavelets3D64` -- against numpy.roll and tests/volume_spin_ref.py, which
tests/test_volume_spin_ref_cpu.py pins.

Bit for bit: every shift (pure data movement), the coefficients of a cycle-spinning handle against a plain handle fed the rolled
volume, and `cycle_spin` with the one shift (0, 0, 0) against forward + threshold + inverse (the weight is 1).

Within a tolerance: `cycle_spin` over the eight lattice shifts, volume_spin_ref.CASES.  fp32: K_TOL = 4 times the distance between
the fp32 composition and the fp64-accumulated one (tests/test_volume_spin_ref_cpu.py derives it and proves that one voxel of a wrong
unshift is at least 100 tolerances away), against the fp64-accumulated composition; fp64: 1e-12 max |ref| against the fp64
composition.  The largest error over tolerance of every case is kept; test_report prints the table
(profiles/volume_spin_parity.txt is the MI355X run's; PDWT_VOLUME_SPIN_PARITY_OUT=<file> writes it, as the tap tests do).
Measured there: largest error over tolerance 0.52 in fp32 (5 x 7 x 11 haar, soft) and 0.002 in fp64.
"""
import ctypes as C
import os

import numpy as np
import pytest

import volume_spin_ref as spin
from oracle import oracle

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHIFT_SHAPES = [(8, 8, 16), (5, 7, 11), (9, 10, 12)]
SHIFTS = [(0, 0, 0), (1, 0, 0), (0, -3, 5), (-13, 27, -40)]
RATIOS = {}


@pytest.fixture(scope="module")
def classes():
    oracle.build()
    from pypwt_amd import Wavelets3D, Wavelets3D64
    return {np.float32: Wavelets3D, np.float64: Wavelets3D64}


def data(shape, dtype, seed=0):
    return np.random.default_rng(100 * sum(shape) + seed).uniform(0.0, 255.0, shape).astype(np.float32).astype(dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- circshift

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("swt", [0, 1])
def test_circshift_is_numpy_roll_bit_for_bit_in_place_and_composes(classes, dtype, swt):
    for shape in SHIFT_SHAPES:
        x = data(shape, dtype)
        W = classes[dtype](x, "haar", 1, do_swt=swt)
        ptr = W._lib.pdwt_volume_image_ptr(W._h)
        # (8, 8, 16): sc = 4 moves groups both ways, sc = 3 stores groups and loads values; the other shapes go value by value
        for s in SHIFTS + [(0, 0, 4), (0, 0, 3), (2, 1, 4), (1, 2, 3)]:
            W.set_image(x)
            W.circshift(*s)
            assert same_bits(W.image, spin.shift(x, s)), (shape, s)
            assert W._lib.pdwt_volume_image_ptr(W._h) == ptr
        W.set_image(x)
        W.circshift(1, 2, 3)
        W.circshift(-4, 9, 5)
        assert same_bits(W.image, spin.shift(x, (-3, 11, 8))), shape
        # the shifted image is an image like any other: the transform of it round-trips, and the result can be shifted again
        W.forward()
        W.inverse()
        W.circshift(3, -11, -8)
        back = W.image
        assert float(np.abs(back - x).max()) <= (1e-3 if dtype == np.float32 else 1e-10), shape


@pytest.mark.parametrize("dtype", DTYPES)
def test_circshift_after_forward_is_refused_and_changes_nothing(classes, dtype):
    from pypwt_amd import _lib
    x = data((9, 10, 12), dtype)
    for swt in (0, 1):
        W = classes[dtype](x, "db2", 1, do_swt=swt)
        W.forward()
        coeffs = [W.coeff_only(k) for k in range(W.nbands)]
        assert W._lib.pdwt_volume_circshift(W._h, 1, 2, 3) == _lib.ERR_STATE
        assert all(same_bits(W.coeff_only(k), c) for k, c in enumerate(coeffs))
        assert same_bits(W.image, x)
    assert W._lib.pdwt_volume_circshift(None, 1, 2, 3) == _lib.ERR_ARG


# -------------------------------------------------------------------------------------------------------- do_cycle_spinning

@pytest.mark.parametrize("dtype", DTYPES)
def test_cycle_spinning_forward_shifts_and_inverse_shifts_back(classes, dtype):
    cls = classes[dtype]
    shape = (9, 10, 12)
    x = data(shape, dtype, 1)
    plain = cls(x, "db2", 1)
    assert plain.last_shift == (0, 0, 0)
    plain.forward()
    assert plain.last_shift == (0, 0, 0)
    W = cls(x, "db2", 1).set_cycle_spinning(1, seed=12345)
    twin = cls(x, "db2", 1).set_cycle_spinning(1, seed=12345)
    other = cls(x, "db2", 1).set_cycle_spinning(1, seed=54321)
    assert W.do_cycle_spinning == 1 and plain.do_cycle_spinning == 0
    assert W.last_shift == (0, 0, 0)
    draws, other_draws = [], []
    for _ in range(3):
        W.set_image(x)
        W.forward()
        s = W.last_shift
        draws.append(s)
        assert all(0 <= v < n for v, n in zip(s, shape))
        twin.forward(x)
        assert twin.last_shift == s  # the same seed: the same draws
        other.forward(x)
        other_draws.append(other.last_shift)
        rolled = spin.shift(x, s)
        plain.forward(rolled)
        for k in range(W.nbands):
            assert same_bits(W.coeff_only(k), plain.coeff_only(k)), (s, k)
        W.soft_threshold(20.0)
        plain.soft_threshold(20.0)
        W.inverse()
        plain.inverse()
        assert W.last_shift == (0, 0, 0)
        assert same_bits(W.image, spin.shift(plain.image, [-v for v in s])), s
        other.inverse()
        twin.inverse()
    assert len(set(draws)) > 1 and draws != other_draws
    # forwards in a row: the shifts add up, and one inverse undoes them all
    W.set_image(x)
    W.forward()
    first = W.last_shift
    W.forward()
    total = W.last_shift
    plain.forward(spin.shift(x, total))
    assert total != first and all(same_bits(W.coeff_only(k), plain.coeff_only(k)) for k in range(W.nbands))
    W.inverse()
    plain.inverse()
    assert same_bits(W.image, spin.shift(plain.image, [-v for v in total]))


def test_cycle_spinning_is_refused_on_a_stationary_volume(classes):
    from pypwt_amd import _lib
    x = data((8, 8, 16), np.float32)
    W = classes[np.float32](x, "haar", 1, do_swt=1)
    assert W._lib.pdwt_volume_set_cycle_spinning(W._h, 1, 7) == _lib.ERR_UNSUPPORTED
    W.forward()
    assert W.last_shift == (0, 0, 0)
    W.inverse()
    with pytest.raises(NotImplementedError):
        W.set_cycle_spinning(1, seed=7)
    assert W.do_cycle_spinning == 0


# ----------------------------------------------------------------------------------------------------------------- cycle_spin

@pytest.mark.parametrize("dtype", DTYPES)
def test_one_shift_of_zero_is_the_plain_denoiser_bit_for_bit(classes, dtype):
    cls = classes[dtype]
    for shape, wname, levels in spin.SHAPES:
        x = data(shape, dtype, 2)
        for mode, do_app in (("soft", 0), ("hard", 1)):
            plain = cls(x, wname, levels)
            plain.forward()
            getattr(plain, mode + "_threshold")(spin.BETA, do_app)
            plain.inverse()
            W = cls(x, wname, levels)
            assert W.cycle_spin(shifts=[(0, 0, 0)], mode=mode, beta=spin.BETA, do_threshold_appcoeffs=do_app) is W
            assert same_bits(W.image, plain.image), (shape, mode)
            assert W.info()["state"] == plain.info()["state"]
            # n = 1 of the lattice is that shift too
            V = cls(x, wname, levels)
            V.cycle_spin(n=1, mode=mode, beta=spin.BETA, do_threshold_appcoeffs=do_app)
            assert same_bits(V.image, plain.image)


@pytest.mark.parametrize("case", spin.CASES, ids=spin.case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_eight_shifts_against_the_reference(classes, dtype, case):
    shape, wname, levels, mode, do_app, method = case
    x = spin.case_input(case, dtype)
    W = classes[dtype](x, wname, levels)
    kw = dict(method=method) if method else dict(beta=spin.BETA, do_threshold_appcoeffs=do_app)
    W.cycle_spin(n=8, mode=mode, **kw)
    got = W.image
    if dtype == np.float32:
        ref, tol = spin.tolerance(case)
    else:
        ref = spin.run_case(case, "full", dtype=np.float64)
        tol = 1e-12 * float(np.abs(ref).max())
    err = float(np.abs(got.astype(np.float64) - ref).max())
    RATIOS[(np.dtype(dtype).name, spin.case_id(case))] = err / tol
    print("volume-spin %s %s: err %.3g tol %.3g err/tol %.2f" % (np.dtype(dtype).name, spin.case_id(case), err, tol, err / tol))
    assert err <= tol, (err, tol)
    # explicit shifts are the lattice's
    V = classes[dtype](x, wname, levels)
    V.cycle_spin(shifts=spin.lattice(8), mode=mode, **kw)
    assert same_bits(V.image, got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_second_cycle_spin_gives_the_same_bits_and_the_handle_stays_a_plain_one(classes, dtype):
    cls = classes[dtype]
    shape, wname, levels = spin.SHAPES[0]
    x, y = data(shape, dtype, 3), data(shape, dtype, 4)
    W = cls(x, wname, levels)
    W.cycle_spin(n=8, beta=spin.BETA)
    first = W.image
    W.set_image(y)
    W.cycle_spin(n=4, beta=spin.BETA)  # something else in between: the running mean starts afresh every time
    W.set_image(x)
    W.cycle_spin(n=8, beta=spin.BETA)
    assert same_bits(W.image, first)
    # the result is the image of a volume after inverse(): it can be spun again without set_image ...
    W.cycle_spin(n=1, beta=0.0)
    again = W.image
    assert float(np.abs(again - first).max()) <= (1e-3 if dtype == np.float32 else 1e-10)
    # ... and a plain forward / inverse behaves as on a fresh handle
    fresh = cls(y, wname, levels)
    fresh.forward()
    W.forward(y)
    assert W.last_shift == (0, 0, 0)
    assert all(same_bits(W.coeff_only(k), fresh.coeff_only(k)) for k in range(W.nbands))
    fresh.soft_threshold(10.0)
    W.soft_threshold(10.0)
    fresh.inverse()
    W.inverse()
    assert same_bits(W.image, fresh.image)


def test_cycle_spin_refusals_leave_the_image_alone(classes):
    from pypwt_amd import _lib
    x = data((9, 10, 12), np.float32, 5)
    lattice = np.ascontiguousarray(spin.lattice(8), dtype=np.int32)
    sh = lattice.ctypes.data_as(C.POINTER(C.c_int))

    def spin_rc(W, nshifts=8, shifts=sh, op=0, method=-1):
        return W._lib.pdwt_volume_cycle_spin_async(W._h, nshifts, shifts, op, spin.BETA, 0, 0, method, None, 1)

    W = classes[np.float32](x, "db2", 1)
    # arguments
    assert spin_rc(W, nshifts=0) == _lib.ERR_ARG
    assert spin_rc(W, shifts=None) == _lib.ERR_ARG
    assert spin_rc(W, op=2) == _lib.ERR_ARG
    assert spin_rc(W, method=2) == _lib.ERR_ARG
    assert W._lib.pdwt_volume_cycle_spin_async(None, 8, sh, 0, spin.BETA, 0, 0, -1, None, 1) == _lib.ERR_ARG
    assert same_bits(W.image, x) and W.info()["state"] == 0  # (PDWT_INIT)
    for kw in (dict(), dict(beta=1.0, method="BayesShrink")):
        with pytest.raises(ValueError):
            W.cycle_spin(**kw)
    with pytest.raises(ValueError):
        W.cycle_spin(beta=1.0, shifts=[(0, 0)])
    with pytest.raises(ValueError):
        W.cycle_spin(beta=1.0, shifts=[(0.5, 0.0, 0.0)])
    with pytest.raises(ValueError):
        W.cycle_spin(beta=1.0, mode="medium")
    assert same_bits(W.image, x)
    # after forward() the image is not current
    W.forward()
    coeffs = [W.coeff_only(k) for k in range(W.nbands)]
    assert spin_rc(W) == _lib.ERR_STATE
    assert all(same_bits(W.coeff_only(k), c) for k, c in enumerate(coeffs)) and same_bits(W.image, x)
    W.inverse()  # ... after inverse() it is again
    assert spin_rc(W) == _lib.OK
    # a stationary volume
    S = classes[np.float32](x, "db2", 1, do_swt=1)
    assert spin_rc(S) == _lib.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        S.cycle_spin(beta=1.0)
    assert same_bits(S.image, x)
    # a volume that draws its own shifts
    R = classes[np.float32](x, "db2", 1).set_cycle_spinning(1, seed=1)
    assert spin_rc(R) == _lib.ERR_STATE
    assert same_bits(R.image, x) and R.last_shift == (0, 0, 0)


def test_spin_footprint_is_two_aligned_volumes(classes):
    from pypwt_amd import _lib
    from pypwt_amd.volume import spin_footprint

    def aligned(n):
        return (n + 255) // 256 * 256
    for shape in [(9, 10, 12), (8, 8, 16), (5, 7, 11), (256, 256, 256), (512, 511, 511)]:
        n = shape[0] * shape[1] * shape[2]
        assert spin_footprint(shape, np.float32) == 2 * aligned(4 * n)
        assert spin_footprint(shape, np.float64) == 2 * aligned(8 * n)
    lib = _lib.load()
    out = C.c_size_t(0)
    assert lib.pdwt_volume_spin_footprint(0, 8, 8, 4, C.byref(out)) == _lib.ERR_ARG
    assert lib.pdwt_volume_spin_footprint(8, 8, 8, 3, C.byref(out)) == _lib.ERR_ARG
    assert lib.pdwt_volume_spin_footprint(8, 8, 8, 4, None) == _lib.ERR_ARG
    assert lib.pdwt_volume_spin_footprint(8, 8, 8, 0, C.byref(out)) == _lib.OK and out.value == 2 * aligned(4 * 512)


# -------------------------------------------------------------------------------------------------------------- report

def test_report():
    """Closes the module: every tolerance case ran in both precisions; prints the table of profiles/volume_spin_parity.txt."""
    assert len(RATIOS) == 2 * len(spin.CASES), len(RATIOS)
    lines = ["volume-spin-parity  cycle_spin over the 8 lattice shifts, max |gpu - ref| over the tolerance.  fp32: tolerance = %d x max |fp32 "
             "composition - fp64-accumulated composition|," % spin.K_TOL,
             "volume-spin-parity  against the fp64-accumulated composition; fp64: tolerance = 1e-12 max |ref|, against the fp64 composition"]
    for prec in ("float32", "float64"):
        for case in spin.CASES:
            lines.append("volume-spin-parity  %s %-36s %.3f" % (prec, spin.case_id(case), RATIOS[(prec, spin.case_id(case))]))
        lines.append("volume-spin-parity  %s largest: %.3f" % (prec, max(v for k, v in RATIOS.items() if k[0] == prec)))
    print("\n" + "\n".join(lines))
    if os.environ.get("PDWT_VOLUME_SPIN_PARITY_OUT"):  # how profiles/volume_spin_parity.txt is made
        with open(os.environ["PDWT_VOLUME_SPIN_PARITY_OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")
