"""The resolving power of tests/test_gpu_volume_taps.py, proved on the CPU with the composition of the oracle alone
(tests/volume_ref.py): with a bank of tap_banks.bank on all three axes, zeroing ANY single tap of any of the four filters in the DEPTH
step only moves the one-level composition by at least 1000 x the tolerance the GPU module compares the volumes at -- so a depth kernel
that drops, shifts or mis-stages one tap cannot pass, at either of the module's two shapes, and K cannot be raised into blindness.
The last test pins why the module exists: with db20's own taps and tests/test_gpu_volume.py's bound, zeroing the smallest dec_lo tap
of the depth step goes unseen."""
import numpy as np
import pytest

from oracle import oracle
import tap_banks
import volume_ref

LENGTHS = (4, 6, 16, 18, 22, 40)
MIN_FACTOR = 1000.0


@pytest.fixture(scope="module", autouse=True)
def one_oracle_thread():
    """Thousands of oracle runs on planes of a hundred samples: a team of threads per run costs more than the run."""
    libs = [oracle.load(False), oracle.load(True)]
    prev = [lib.oracle_set_threads(0) for lib in libs]
    for lib in libs:
        lib.oracle_set_threads(1)
    yield
    for lib, n in zip(libs, prev):
        lib.oracle_set_threads(n)


def smallest_factor(n, shape, filt, x, k=None):
    """The smallest, over every single tap of the four filters, of (change of the f64acc composition when that tap is zeroed in the
    depth step) / tolerance; the forward for dec_lo / dec_hi, the inverse of the forward reference's coefficients for rec_lo / rec_hi."""
    ref, tols = tap_banks.volume_forward_reference(x, filt, k=k)
    for (tol, noise), r in zip(tols, ref):
        assert 0 < noise <= 1e-6 * float(np.abs(r).max()), (n, shape, noise)
    iref, (itol, inoise) = tap_banks.volume_inverse_reference(ref, shape, filt, k=k)
    assert 0 < inoise <= 1e-6 * float(np.abs(iref).max()), (n, shape, inoise)
    worst = np.inf
    for which in (1, 2):
        for j in range(n):
            factor = tap_banks.depth_tap_factor(x, filt, which, j, ref, tols)
            worst = min(worst, factor)
            assert factor >= MIN_FACTOR, (n, shape, "forward", which, j, factor)
    for which in (3, 4):
        for j in range(n):
            got = volume_ref.inverse(ref, shape, None, 1, True, filt=filt, depth_filt=tap_banks.without_tap(filt, which, j))
            factor = float(np.abs(got.astype(np.float64) - iref).max()) / itol
            worst = min(worst, factor)
            assert factor >= MIN_FACTOR, (n, shape, "inverse", which, j, factor)
    return worst


@pytest.mark.parametrize("n", LENGTHS)
def test_every_single_depth_tap_is_resolved_in_both_directions(n):
    filt = tap_banks.bank(n, 300 + n)
    for i, shape in enumerate(tap_banks.volume_shapes(n)):
        worst = smallest_factor(n, shape, filt, tap_banks.volume_input(shape, 500 + 2 * n + i))
        print("tap-resolved volume n=%d %s: smallest change / tolerance = %.0f (K = %g)" % (n, shape, worst, tap_banks.K))


def test_the_bound_still_holds_at_the_largest_k_allowed():
    """K may be raised to 16 at the most (tap_banks.K_MAX): even then every depth tap of a 40-tap bank is seen 1000 times over."""
    filt = tap_banks.bank(40, 340)
    for i, shape in enumerate(tap_banks.volume_shapes(40)):
        worst = smallest_factor(40, shape, filt, tap_banks.volume_input(shape, 580 + i), k=tap_banks.K_MAX)
        print("tap-resolved volume n=40 %s at K = %g: smallest change / tolerance = %.0f" % (shape, tap_banks.K_MAX, worst))


def test_db20_smallest_depth_tap_is_invisible_to_the_usual_tolerance():
    """Why tests/test_gpu_volume_taps.py exists: db20's smallest dec_lo tap (2e-10) can be zeroed in the depth step of a (40, 40, 44)
    volume and every band stays inside a tenth of tests/test_gpu_volume.py's 1.5e-6 (1 + L) max(max|ref|, 1)."""
    filt = oracle.filters("db20")
    j = int(np.argmin(np.abs(filt[1])))
    assert abs(float(filt[1][j])) < 1e-9
    x = tap_banks.volume_input((40, 40, 44), 9317)
    ref = volume_ref.forward(x, "db20", 1, True)
    got = volume_ref.forward(x, "db20", 1, True, depth_filt=tap_banks.without_tap(filt, 1, j))
    for g, r in zip(got, ref):
        tol = 1.5e-6 * 2 * max(float(np.abs(r).max()), 1.0)
        assert float(np.abs(g.astype(np.float64) - r).max()) <= 0.1 * tol
