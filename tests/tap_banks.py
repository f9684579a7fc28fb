"""Filter banks whose every tap counts, and the tolerance that resolves them (tests/test_tap_banks_cpu.py, tests/test_gpu_taps.py).

The built-in long wavelets have taps far below what an absolute tolerance of 2e-6 (1 + L) max(|band|, 255) can see (db20: 9 of 40 taps
of dec_lo, the smallest 2e-10), so a kernel that dropped one would pass.  bank(n, seed) draws four INDEPENDENT filters of n taps, every
tap sign * u / sqrt(n) with u uniform in [0.5, 1]: no tap below 0.5 / sqrt(40) = 0.079, an L2 norm of at most 1 per filter (three levels
stay far from fp32 overflow), no quadrature-mirror structure a kernel could lean on or a forward bug could cancel against.

The tolerance comes from the reference alone: the oracle runs twice with the same bank, in fp32 arithmetic and with fp64 accumulation
on fp32 data; noise = max |f32 - f64acc| per band is the size of the error a correct fp32 evaluation makes (the kernels differ from
the fp32 oracle in summation order and fma contraction only).  A kernel is compared with the f64acc result at K * noise, floored at
one fp32 ulp of the band's maximum.

K = 4.  The largest err / noise measured on the MI355X is 2.50 (the inverse strip kernels; every family and direction:
profiles/taps_parity.txt); through the depth kernels of a volume it is 2.00 (every even length 4-40, both widths, both directions, forced
depth segments: profiles/volume_taps_parity.txt), through the a-trous depth kernels of a stationary volume 1.75 (every even length 2-40,
every width of both directions, dilations 1-4: profiles/volume_swt_taps_parity.txt).  So 4 holds.  (K may be raised to twice the largest ratio a correct kernel needs, never beyond 16;
tests/test_tap_banks_cpu.py, tests/test_volume_taps_cpu.py and tests/test_volume_swt_taps_cpu.py demand that zeroing any single tap still moves the oracle by 1000 x the
tolerance, whatever K is.)

The volume_* helpers below are the same rule for one level of a volume: the composition of tests/volume_ref.py in the place of the oracle;
the volume_swt_* helpers for any number of levels of a stationary volume: the per-axis composition of tests/volume_swt_ref.py."""
import numpy as np

from oracle import oracle
import volume_ref
import volume_swt_ref

K = 4.0
K_MAX = 16.0
assert K <= K_MAX


def bank(n, seed):
    """(n, dec_lo, dec_hi, rec_lo, rec_hi) as float32: every tap sign * u / sqrt(n), u uniform in [0.5, 1]."""
    rng = np.random.default_rng([int(n), int(seed)])
    taps = []
    for _ in range(4):
        u = rng.uniform(0.5, 1.0, n)
        sign = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
        taps.append((sign * u / np.sqrt(n)).astype(np.float32))
    return (int(n),) + tuple(taps)


def without_tap(filt, which, j):
    """The bank with tap j of filter `which` (1 dec_lo, 2 dec_hi, 3 rec_lo, 4 rec_hi) set to zero."""
    out = [filt[0]] + [f.copy() for f in filt[1:]]
    out[which][j] = 0
    return tuple(out)


def _tol(ref, f32, k):
    noise = float(np.abs(f32.astype(np.float64) - ref).max())
    floor = float(np.spacing(np.float32(np.abs(ref).max())))
    return max(k * noise, floor), noise


def forward_reference(x, levels, filt, ndim=2, do_swt=0, k=None):
    """The f64acc oracle's bands of x, and per band (tolerance, noise): noise = max |fp32 oracle - f64acc oracle|."""
    k = K if k is None else k
    ref = oracle.forward(x, None, levels, ndim=ndim, do_swt=do_swt, double=True, filt=filt)
    f32 = oracle.forward(x, None, levels, ndim=ndim, do_swt=do_swt, double=False, filt=filt)
    return ref, [_tol(r, f, k) for r, f in zip(ref, f32)]


def inverse_reference(bands, shape, levels, filt, ndim=2, do_swt=0, k=None):
    """The f64acc oracle's synthesis of `bands` (fp32 arrays, e.g. forward_reference's), and its (tolerance, noise)."""
    k = K if k is None else k
    ref = oracle.inverse(bands, shape, None, levels, ndim=ndim, do_swt=do_swt, double=True, filt=filt)
    f32 = oracle.inverse(bands, shape, None, levels, ndim=ndim, do_swt=do_swt, double=False, filt=filt)
    return ref, _tol(ref, f32, k)


def assert_forward(bands, x, levels, filt, cap, tag, ndim=2, do_swt=0):
    """Kernel bands (flat list, the oracle's order) against forward_reference at its tolerance, `cap` * max(|band|, 1) at the most;
    returns the reference bands."""
    ref, tols = forward_reference(x, levels, filt, ndim=ndim, do_swt=do_swt)
    assert len(bands) == len(ref), tag
    for k, (g, r, (tol, noise)) in enumerate(zip(bands, ref, tols)):
        err = float(np.abs(np.asarray(g).reshape(r.shape).astype(np.float64) - r).max())
        assert err <= min(tol, cap * max(float(np.abs(r).max()), 1.0)), (tag, k, err, tol, noise)
    return ref


def assert_inverse(w, ref, levels, filt, cap, tag, ndim=2, do_swt=0):
    """The inverse on its own: loads the reference bands into the plan `w` (set_coeff), inverts, and compares with inverse_reference at
    its tolerance, `cap` * max(|image|, 1) at the most."""
    for k, r in enumerate(ref):
        w.set_coeff(r, k)
    w.inverse()
    got = np.asarray(w.image)
    want, (tol, noise) = inverse_reference(ref, got.shape if got.ndim == 2 else (1, got.size), levels, filt, ndim=ndim, do_swt=do_swt)
    err = float(np.abs(got.reshape(want.shape).astype(np.float64) - want).max())
    assert err <= min(tol, cap * max(float(np.abs(want).max()), 1.0)), (tag, err, tol, noise)


# ---- volumes: one level of Wavelets3D (tests/test_volume_taps_cpu.py, tests/test_gpu_volume_taps.py) -----------------------------

def volume_shapes(n):
    """The two volumes an n-tap depth kernel is run on.  A: an odd depth of at least n slices, planes of 96 samples (whole 16-B groups:
    the wide access); B: a depth below the filter length (the source counter wraps up to six times per window at 40 taps), planes
    of 99 samples (one column per lane)."""
    return (n + 7, 8, 12), (3 if n < 8 else 7, 9, 11)


def volume_input(shape, seed):
    return oracle.hash_input(shape, seed)


def volume_forward_reference(x, filt, k=None, depth_filt=None):
    """One level of the f64acc composition (tests/volume_ref.py) with `filt` on all three axes: its eight bands in `num` order, and
    per band (tolerance, noise) with noise = max |fp32 composition - f64acc composition|."""
    k = K if k is None else k
    ref = volume_ref.forward(x, None, 1, True, filt=filt, depth_filt=depth_filt)
    f32 = volume_ref.forward(x, None, 1, False, filt=filt, depth_filt=depth_filt)
    return ref, [_tol(r, f, k) for r, f in zip(ref, f32)]


def volume_inverse_reference(bands, shape, filt, k=None, depth_filt=None):
    """The f64acc composition's synthesis of `bands` (fp32 arrays, e.g. volume_forward_reference's), and its (tolerance, noise)."""
    k = K if k is None else k
    ref = volume_ref.inverse(bands, shape, None, 1, True, filt=filt, depth_filt=depth_filt)
    f32 = volume_ref.inverse(bands, shape, None, 1, False, filt=filt, depth_filt=depth_filt)
    return ref, _tol(ref, f32, k)


def depth_tap_factor(x, filt, which, j, ref, tols):
    """Zeroing tap j of dec_lo (which = 1) or dec_hi (2) in the DEPTH step alone moves the f64acc composition by this many
    tolerances in the band it moves most; ref, tols: volume_forward_reference(x, filt)."""
    got = volume_ref.forward(x, None, 1, True, filt=filt, depth_filt=without_tap(filt, which, j))
    return max(float(np.abs(g.astype(np.float64) - r).max()) / tol for g, r, (tol, _) in zip(got, ref, tols))


# ---- stationary volumes: `levels` levels of Wavelets3D(..., do_swt=1) (tests/test_volume_swt_taps_cpu.py, tests/test_gpu_volume_swt_taps.py)

# (taps, shape, levels): the smallest volumes that reach a dilation above 1 -- the level clamp wants min(shape) >= 2^L (n - 1)
SWT_DILATED = ((4, (25, 24, 28), 3),    # dilation 4; odd depth: one orbit at every level
               (10, (37, 36, 40), 2),   # the inverse on half the forward's columns
               (18, (69, 68, 72), 2),   # taps staged in LDS; the inverse on one column
               (4, (24, 25, 27), 3))    # depth 24: 2 and 4 orbits at dilations 2 and 4; planes of 675 samples, one column per lane


def swt_dilated_input(index):
    """(bank, volume) of SWT_DILATED[index]."""
    n, shape, _ = SWT_DILATED[index]
    return bank(n, 2000 + n), volume_input(shape, 4300 + index)


def volume_swt_forward_reference(x, levels, filt, k=None, depth_filt=None):
    """`levels` levels of the f64acc per-axis composition (tests/volume_swt_ref.py, double=True) with `filt` on all three axes: its
    1 + 7 levels bands in `num` order, and per band (tolerance, noise) with noise = max |fp32 composition - f64acc composition|."""
    k = K if k is None else k
    ref = volume_swt_ref.forward(x, None, levels, True, filt=filt, depth_filt=depth_filt)
    f32 = volume_swt_ref.forward(x, None, levels, False, filt=filt, depth_filt=depth_filt)
    return ref, [_tol(r, f, k) for r, f in zip(ref, f32)]


def volume_swt_inverse_reference(bands, levels, filt, k=None, depth_filt=None):
    """The f64acc composition's synthesis of `bands` (fp32 arrays, e.g. volume_swt_forward_reference's), and its (tolerance, noise)."""
    k = K if k is None else k
    ref = volume_swt_ref.inverse(bands, None, levels, True, filt=filt, depth_filt=depth_filt)
    f32 = volume_swt_ref.inverse(bands, None, levels, False, filt=filt, depth_filt=depth_filt)
    return ref, _tol(ref, f32, k)


def swt_depth_tap_factor(x, levels, filt, which, j, ref, tols, iref=None, itol=None):
    """Zeroing tap j of filter `which` in the DEPTH steps alone moves the f64acc composition by this many tolerances.  dec_lo (1) /
    dec_hi (2): the forward of x, in the band it moves most; ref, tols: volume_swt_forward_reference(x, levels, filt).  rec_lo (3) /
    rec_hi (4): the inverse of `ref`, the reference's own bands; iref, itol: volume_swt_inverse_reference(ref, levels, filt)."""
    cut = without_tap(filt, which, j)
    if which in (1, 2):
        got = volume_swt_ref.forward(x, None, levels, True, filt=filt, depth_filt=cut)
        return max(float(np.abs(g.astype(np.float64) - r).max()) / tol for g, r, (tol, _) in zip(got, ref, tols))
    got = volume_swt_ref.inverse(ref, None, levels, True, filt=filt, depth_filt=cut)
    return float(np.abs(got.astype(np.float64) - iref).max()) / itol
