"""The resolving power of tests/test_gpu_volume_swt_taps.py, proved on the CPU with the per-axis composition alone
(tests/volume_swt_ref.py): with a bank of tap_banks.bank on all three axes, zeroing ANY single tap of any of the four filters in the
DEPTH steps only moves the f64acc composition by at least 1000 x the tolerance the GPU module compares at -- so an a-trous depth
kernel that drops a tap, shifts its register window by one slot or mis-stages a tap in LDS cannot pass, and K cannot be raised into
blindness.

  * level 1: every even length from 2 to 40 taps, both shapes of tap_banks.volume_shapes, every tap of dec_lo / dec_hi (the forward)
    and of rec_lo / rec_hi (the inverse of the reference's own bands) -- the banks and volumes the GPU module runs;
  * the dilated cases (tap_banks.SWT_DILATED, two and three levels): taps 0, n / 2 and n - 1 of each of the four filters;
  * the same at the largest K allowed, at 40 taps;
  * and why the module exists: with db20's own taps on (40, 8, 12) -- tests/test_gpu_volume_swt.py's case for that length -- single
    depth taps can be zeroed inside that module's bound.
"""
import numpy as np
import pytest

from oracle import oracle
import tap_banks
import volume_swt_ref as ref

LENGTHS = tuple(range(2, 41, 2))
MIN_FACTOR = 1000.0


@pytest.fixture(scope="module", autouse=True)
def built():
    oracle.build()


def smallest_factor(x, levels, filt, taps, tag, k=None):
    """The smallest change / tolerance over `taps` (None: every tap) of the four filters; asserts each is at least MIN_FACTOR.
    Returns (analysis, synthesis)."""
    n = filt[0]
    fwd, tols = tap_banks.volume_swt_forward_reference(x, levels, filt, k=k)
    for (tol, noise), r in zip(tols, fwd):
        assert 0 < noise <= 1e-6 * float(np.abs(r).max()), (tag, noise)  # the fp32 composition is a correct evaluation: fp32 noise
    inv, (itol, inoise) = tap_banks.volume_swt_inverse_reference(fwd, levels, filt, k=k)
    # (an arbitrary bank reconstructs nothing: the synthesis cancels, so its noise is measured against what went in)
    assert 0 < inoise <= 1e-6 * max(float(np.abs(r).max()) for r in fwd), (tag, inoise)
    worst = {1: np.inf, 2: np.inf, 3: np.inf, 4: np.inf}
    for which in (1, 2, 3, 4):
        for j in (range(n) if taps is None else taps):
            factor = tap_banks.swt_depth_tap_factor(x, levels, filt, which, j, fwd, tols, inv, itol)
            worst[which] = min(worst[which], factor)
            assert factor >= MIN_FACTOR, (tag, which, j, factor)
    return min(worst[1], worst[2]), min(worst[3], worst[4])


@pytest.mark.parametrize("n", LENGTHS)
def test_every_single_depth_tap_is_resolved_at_level_one(n):
    filt = tap_banks.bank(n, 2000 + n)
    for i, shape in enumerate(tap_banks.volume_shapes(n)):
        x = tap_banks.volume_input(shape, 4100 + 2 * n + i)
        ana, syn = smallest_factor(x, 1, filt, None, (n, shape))
        print("tap-resolved stationary volume n=%d %s: smallest change / tolerance = %.0f analysis, %.0f synthesis (K = %g)"
              % (n, shape, ana, syn, tap_banks.K))


@pytest.mark.parametrize("index", range(len(tap_banks.SWT_DILATED)), ids=["%d-%dx%dx%d-L%d" % ((n,) + s + (l,)) for n, s, l in tap_banks.SWT_DILATED])
def test_sampled_depth_taps_are_resolved_through_the_dilated_levels(index):
    n, shape, levels = tap_banks.SWT_DILATED[index]
    assert ref.clamp_levels(shape, n, levels + 1) == levels  # the smallest volume that reaches the dilation: one level more is clamped
    filt, x = tap_banks.swt_dilated_input(index)
    ana, syn = smallest_factor(x, levels, filt, (0, n // 2, n - 1), (n, shape, levels))
    print("tap-resolved stationary volume n=%d %s L=%d: smallest change / tolerance = %.0f analysis, %.0f synthesis"
          % (n, shape, levels, ana, syn))


def test_the_bound_still_holds_at_the_largest_k_allowed():
    """K may be raised to 16 at the most (tap_banks.K_MAX): even then every depth tap of a 40-tap bank is seen 1000 times over."""
    filt = tap_banks.bank(40, 2040)
    for i, shape in enumerate(tap_banks.volume_shapes(40)):
        ana, syn = smallest_factor(tap_banks.volume_input(shape, 4180 + i), 1, filt, None, (40, shape, "K_MAX"), k=tap_banks.K_MAX)
        print("tap-resolved stationary volume n=40 %s at K = %g: %.0f analysis, %.0f synthesis" % (shape, tap_banks.K_MAX, ana, syn))


def test_db20_depth_taps_can_be_zeroed_inside_the_usual_tolerance():
    """Why tests/test_gpu_volume_swt_taps.py exists: db20 on (40, 8, 12), one level -- the case of tests/test_gpu_volume_swt.py for
    40 taps, its data and its rule tol32 = max(1.5e-6 (1 + L) max(max|ref|, 1), 2 |fp32 composition - fp64 composition|).  At least one
    of the 80 analysis taps can be zeroed in the depth step alone with every band inside that rule."""
    shape, levels = (40, 8, 12), 1
    filt = tuple(oracle.filters("db20", np.float32))
    x = np.random.default_rng(1000 * sum(shape) + levels).uniform(0.0, 255.0, shape).astype(np.float32)
    f64 = ref.forward(x, None, levels, "full", filt=filt)
    f32 = ref.forward(x, None, levels, False, filt=filt)
    tols = [max(1.5e-6 * (1 + levels) * max(float(np.abs(a).max()), 1.0), 2.0 * float(np.abs(b.astype(np.float64) - a).max()))
            for a, b in zip(f64, f32)]
    unseen = []
    for which in (1, 2):
        for j in range(40):
            got = ref.forward(x, None, levels, "full", filt=filt, depth_filt=tap_banks.without_tap(filt, which, j))
            if all(float(np.abs(g - r).max()) <= t for g, r, t in zip(got, f64, tols)):
                unseen.append((which, j, float(filt[which][j])))
    print("db20 on %s: %d of 80 analysis taps can be zeroed in the depth step inside tol32: %s" % (shape, len(unseen), unseen))
    assert len(unseen) >= 1
    assert all(abs(t) < 1e-4 for _, _, t in unseen)  # (and they are the small ones: the rule is blind, not wrong)
