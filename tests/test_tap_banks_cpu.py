"""The resolving power of the tap-resolved parity tests (tests/tap_banks.py, tests/test_gpu_taps.py), proved on the CPU with the oracle
alone: with a bank of tap_banks.bank, zeroing ANY single tap of any of the four filters moves the oracle's output by at least 1000 x
the tolerance the GPU module compares kernels at -- so a kernel that drops, shifts or mis-loads one tap cannot pass, and the
tolerance's factor K cannot be raised into blindness.  The last test pins why the module exists: with db20's own taps and the suite's
usual absolute tolerance, zeroing the smallest dec_lo tap goes unseen."""
import numpy as np
import pytest

from oracle import oracle
import tap_banks

# one small shape per transform kind; the 2D DWT one has both axes shorter than 40 taps (the filter wraps)
KINDS = {"dwt2": ((24, 40), 1, 2, 0), "swt2": ((32, 48), 2, 2, 1), "dwt1": ((3, 520), 3, 1, 0), "swt1": ((2, 264), 2, 1, 1)}
MIN_FACTOR = 1000.0


@pytest.fixture(scope="module", autouse=True)
def one_oracle_thread():
    """Hundreds of oracle runs on images of a few thousand samples: a team of threads per run costs more than the run."""
    libs = [oracle.load(False), oracle.load(True)]
    prev = [lib.oracle_set_threads(0) for lib in libs]
    for lib in libs:
        lib.oracle_set_threads(1)
    yield
    for lib, n in zip(libs, prev):
        lib.oracle_set_threads(n)


def _input(shape, seed):
    return oracle.hash_input(shape, seed)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n", [6, 22, 40])
def test_every_single_tap_is_resolved_in_both_directions(n, kind):
    shape, levels, ndim, swt = KINDS[kind]
    filt = tap_banks.bank(n, 100 + n)
    for f in filt[1:]:
        assert f.dtype == np.float32 and np.abs(f).min() >= 0.5 / np.sqrt(n) * (1 - 1e-6) and float(np.sum(f.astype(np.float64) ** 2)) <= 1.0 + 1e-6
    x = _input(shape, 31 + n)
    ref, tols = tap_banks.forward_reference(x, levels, filt, ndim=ndim, do_swt=swt)
    for (tol, noise), r in zip(tols, ref):
        # the oracle's own fp32 error: a few 1e-7 of the band (the issue measured 0.7e-7 .. 4.1e-7)
        assert 0 < noise <= 1e-6 * float(np.abs(r).max()), (kind, n, noise)
    iref, (itol, inoise) = tap_banks.inverse_reference(ref, shape, levels, filt, ndim=ndim, do_swt=swt)
    assert 0 < inoise <= 1e-6 * float(np.abs(iref).max()), (kind, n, inoise)
    worst = np.inf
    for which in (1, 2):      # the analysis filters: the forward transform
        for j in range(n):
            got = oracle.forward(x, None, levels, ndim=ndim, do_swt=swt, double=True, filt=tap_banks.without_tap(filt, which, j))
            factor = max(float(np.abs(g.astype(np.float64) - r).max()) / tol for g, r, (tol, _) in zip(got, ref, tols))
            worst = min(worst, factor)
            assert factor >= MIN_FACTOR, (kind, n, "forward", which, j, factor)
    for which in (3, 4):      # the synthesis filters: the inverse of the same coefficients
        for j in range(n):
            got = oracle.inverse(ref, shape, None, levels, ndim=ndim, do_swt=swt, double=True, filt=tap_banks.without_tap(filt, which, j))
            factor = float(np.abs(got.astype(np.float64) - iref).max()) / itol
            worst = min(worst, factor)
            assert factor >= MIN_FACTOR, (kind, n, "inverse", which, j, factor)
    print("tap-resolved %s n=%d: smallest change / tolerance = %.0f (K = %g)" % (kind, n, worst, tap_banks.K))


def test_the_bound_still_holds_at_the_largest_k_allowed():
    """K may be raised to 16 at the most (tap_banks.K_MAX): even then every tap of a 40-tap bank is seen 1000 times over."""
    shape, levels, ndim, swt = KINDS["dwt2"]
    filt = tap_banks.bank(40, 140)
    x = _input(shape, 71)
    ref, tols = tap_banks.forward_reference(x, levels, filt, k=tap_banks.K_MAX)
    for which in (1, 2):
        for j in range(40):
            got = oracle.forward(x, None, levels, double=True, filt=tap_banks.without_tap(filt, which, j))
            assert max(float(np.abs(g - r).max()) / tol for g, r, (tol, _) in zip(got, ref, tols)) >= MIN_FACTOR, (which, j)


def test_banks_are_reproducible_and_independent():
    a, b = tap_banks.bank(40, 7), tap_banks.bank(40, 7)
    assert all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    assert not np.array_equal(tap_banks.bank(40, 8)[1], a[1])
    for i in range(1, 5):
        for j in range(i + 1, 5):   # no two filters are mirrors, sign flips or copies of each other
            assert not np.allclose(np.abs(a[i]), np.abs(a[j])) and not np.allclose(np.abs(a[i]), np.abs(a[j][::-1]))


def test_db20_smallest_tap_is_invisible_to_the_usual_tolerance():
    """Why tests/test_gpu_taps.py exists: db20's smallest dec_lo tap (2e-10) can be zeroed and the level-1 bands of a 136 x 264 hash
    image stay inside 2e-6 (1 + L) max(|band|, 255) -- by two orders of magnitude."""
    filt = oracle.filters("db20")
    j = int(np.argmin(np.abs(filt[1])))
    assert abs(float(filt[1][j])) < 1e-9
    x = _input((136, 264), 9317)
    ref = oracle.forward(x, "db20", 1, double=True)
    got = oracle.forward(x, "db20", 1, double=True, filt=tap_banks.without_tap(filt, 1, j))
    for g, r in zip(got, ref):
        tol = 2e-6 * 2 * max(float(np.abs(r).max()), 255.0)
        assert float(np.abs(g - r).max()) <= 0.1 * tol
    # ... while the tap-resolved tolerance with a bank of tap_banks sees a tap of the same slot 1000 times over (first test)
