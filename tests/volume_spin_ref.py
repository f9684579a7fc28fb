"""Circular shifts and cycle spinning of a volume in plain numpy (`Wavelets3D.circshift`, `set_cycle_spinning`, `cycle_spin`):
numpy.roll on three axes around the forward / inverse of tests/volume_ref.py, the global thresholds of that module and the
adaptive ones of tests/volume_ops_ref.py.

    cycle_spin(x) = 1/K sum_s roll(inverse(theta(forward(roll(x, s)))), -s)                       (Coifman and Donoho)

`double`: False -- fp32 data, arithmetic and running mean, in the device's order (w x_0, then acc + w x_s); True -- fp32 data with
fp64 accumulation inside the transforms (tests/volume_ref.py) and an fp64 mean, what the fp32 results are compared with; "full" --
fp64 throughout, the checker of the fp64 library.

CASES are the tolerance cases of tests/test_gpu_volume_spin.py; tests/test_volume_spin_ref_cpu.py derives their tolerance from
this module alone and proves that it can tell one voxel of a wrong unshift.
"""
import itertools

import numpy as np

import volume_ops_ref
import volume_ref

BETA = 50.0  # uniform(0, 255) data: the details have a standard deviation of 255 / sqrt(12) = 74; about half of them go
# (shape, wname, levels asked for, mode, do_threshold_appcoeffs, method): db2 gets ONE level on these sizes (the level clamp), haar two
SHAPES = (((9, 10, 12), "db2", 2), ((8, 8, 16), "db2", 2), ((5, 7, 11), "haar", 2))
# The adaptive cases estimate sigma as the median of |ddd_1| WITHOUT its exact zeros (skimage's rule), which is not a continuous
# function of the coefficients where a coefficient is zero by construction: the haar detail of the sample an odd axis repeats is
# x h0 + x h1 = 0 in the reference (two rounded products of opposite sign) and the rounding error of one product, about 1e-6, with
# the device's fused multiply-add -- 42 of the 72 values of ddd_1 on (5, 7, 11).  The two medians are then taken over different
# sets, and no tolerance derived from rounding covers that.  The adaptive cases therefore run where ddd_1 has no zero by
# construction: the two db2 shapes, and haar with two levels on the EVEN (8, 8, 16); tests/test_volume_spin_ref_cpu.py asserts that
# premise for every one of them.
METHOD_SHAPES = (SHAPES[0], SHAPES[1], ((8, 8, 16), "haar", 2))
CASES = ([(shape, wname, levels, mode, do_app, None) for shape, wname, levels in SHAPES for mode in ("soft", "hard") for do_app in (0, 1)]
         + [(shape, wname, levels, "soft", 0, method) for shape, wname, levels in METHOD_SHAPES for method in ("BayesShrink", "VisuShrink")])
K_TOL = 4  # the tolerance is K_TOL times the distance between the fp32 and the fp64-accumulated composition (tests/tap_banks.py: K)


def case_id(case):
    shape, wname, levels, mode, do_app, method = case
    return "%s-%s-L%d-%s-%s" % ("x".join(str(n) for n in shape), wname, levels, mode, method if method else "app%d" % do_app)


def case_input(case, dtype=np.float32):
    """uniform(0, 255), the same for every precision (drawn in float32)."""
    seed = sum(ord(c) for c in case_id(case))
    return np.random.default_rng(seed).uniform(0.0, 255.0, size=case[0]).astype(np.float32).astype(dtype)


def shift(x, s):
    """numpy.roll on (z, y, x): out[z][r][c] = x[z - sz][r - sr][c - sc]."""
    return np.roll(x, tuple(int(v) for v in s), axis=(0, 1, 2))


def lattice(n):
    """The default shifts of `Wavelets3D.cycle_spin`: {0, 1}^3 in lexicographic order, then the rest of {0 .. 3}^3 in that order."""
    first = list(itertools.product((0, 1), repeat=3))
    rest = [p for p in itertools.product(range(4), repeat=3) if max(p) > 1]
    return np.array((first + rest)[:n], dtype=np.int64)


def denoise_once(x, wname, levels, mode="soft", beta=None, method=None, sigma=None, do_app=0, normalize=0, skip_zeros=True, double=False):
    """(inverse(theta(forward(x))), zeroed details, details): one pass of the decimated denoiser; `levels` is clamped here."""
    L = volume_ref.clamp_levels(x.shape, volume_ref.hlen_of(wname), levels)
    bands = volume_ref.forward(x, wname, L, double)
    if method is None:
        bands = volume_ref.threshold(bands, L, mode, beta, do_app, normalize)
    else:
        bands = volume_ops_ref.denoise(bands, x.shape, method, mode, sigma, skip_zeros)[2]
    zeroed = sum(int(np.count_nonzero(b == 0)) for b in bands[1:])
    return volume_ref.inverse(bands, x.shape, wname, L, double), zeroed, sum(b.size for b in bands[1:])


def mean_of(recs, shifts, double=False):
    """The running mean of the reconstructions, each shifted back by its shift, in the device's order."""
    k = len(recs)
    if double is False:
        w = np.float32(1.0 / k)
        acc = None
        for rec, s in zip(recs, shifts):
            term = w * shift(np.asarray(rec, dtype=np.float32), [-v for v in s])
            acc = term if acc is None else acc + term
        return acc
    acc = np.zeros(recs[0].shape, dtype=np.float64)
    for rec, s in zip(recs, shifts):
        acc = acc + (1.0 / k) * shift(np.asarray(rec, dtype=np.float64), [-v for v in s])
    return acc


def cycle_spin(x, wname, levels, shifts, mode="soft", beta=None, method=None, sigma=None, do_app=0, normalize=0, skip_zeros=True,
               double=False, parts=False):
    """The mean over `shifts` ((K, 3) integers).  With `parts`: (mean, the K reconstructions before their unshift, the share of the
    detail coefficients the operator zeroed)."""
    x = np.ascontiguousarray(x, dtype=np.float64 if double == "full" else np.float32)
    recs, zeroed, total = [], 0, 0
    for s in shifts:
        rec, z, t = denoise_once(shift(x, s), wname, levels, mode, beta, method, sigma, do_app, normalize, skip_zeros, double)
        recs.append(rec)
        zeroed += z
        total += t
    out = mean_of(recs, shifts, double)
    return (out, recs, zeroed / float(total)) if parts else out


def run_case(case, double, parts=False, dtype=np.float32):
    shape, wname, levels, mode, do_app, method = case
    x = case_input(case, dtype)
    return cycle_spin(x, wname, levels, lattice(8), mode, None if method else BETA, method, None, do_app, 0, True, double, parts)


_tolerances = {}


def tolerance(case):
    """(the fp64-accumulated reference, K_TOL max |fp32 composition - it|) of a case: computed once."""
    key = case_id(case)
    if key not in _tolerances:
        ref = run_case(case, True)
        f32 = run_case(case, False)
        _tolerances[key] = (ref, K_TOL * float(np.abs(f32.astype(np.float64) - ref).max()))
    return _tolerances[key]
