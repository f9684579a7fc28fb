"""Plain numpy references of the coefficient operators, restated from the semantics block at the top of
pypwt_amd/csrc/ops_kernels.hpp and from the drivers in plan.cpp (threshold_sweep, app_beta, pdwt_shrink,
pdwt_group_soft_threshold, pdwt_add_wavelet, the norms).  They work on a list of bands in the plan's order -- band 0 is the
approximation, then the detail bands level by level (three per level in 2D, one in 1D) -- for float32 and float64 bands.  The
band's dtype is the library's `real_t`: every scalar the C code keeps in a `real_t` is rounded to it here.

tests/test_ops_ref_cpu.py pins the float32 forms to the committed C oracle bit for bit, so the GPU tests can use these at sizes
and in types the oracle's Python wrapper does not take.
"""
import math

import numpy as np

SQRT_2 = 1.4142135623730951  # the double the C code divides by


def per_level(ndim):
    return 3 if ndim == 2 else 1


def app_beta(beta, levels, normalize, dtype):
    """beta of the approximation band: beta / sqrt(2)^levels as a power of two and one optional division (plan.cpp: app_beta)."""
    beta = dtype(beta)
    if normalize > 0:
        n2 = levels // 2
        beta = dtype(beta / dtype(1 << n2))
        if n2 * 2 != levels:
            beta = dtype(np.float64(beta) / SQRT_2) if dtype is np.float32 else dtype(beta / SQRT_2)
    return beta


def level_betas(beta, levels, normalize, dtype):
    """beta of the detail bands of level 1 .. levels: divided by the double 1.4142135623730951 once per level and rounded to the
    band's type after every step when `normalize`, else beta itself."""
    out = []
    b = dtype(beta)
    for _ in range(levels):
        if normalize > 0:
            b = dtype(np.float64(b) / SQRT_2)
        out.append(b)
    return out


def soft(x, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.copysign(np.fmax(np.abs(x) - x.dtype.type(b), x.dtype.type(0)), x)


def hard(x, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > x.dtype.type(b), x, x.dtype.type(0))


def linf(x, b):
    with np.errstate(invalid="ignore"):
        return np.copysign(np.fmin(np.abs(x), x.dtype.type(b)), x)


_EW = {"soft": soft, "hard": hard, "linf": linf}


def threshold(bands, levels, ndim, op, beta, do_app=0, normalize=0):
    """soft / hard / linf on every detail band, and on the approximation band when `do_app`; `linf` takes no `normalize`."""
    dt = bands[0].dtype.type
    per = per_level(ndim)
    assert len(bands) == per * levels + 1
    if op == "linf":
        normalize = 0
    fn = _EW[op]
    out = [fn(bands[0], app_beta(beta, levels, normalize, dt)) if do_app else bands[0].copy()]
    betas = level_betas(beta, levels, normalize, dt)
    for l in range(1, levels + 1):
        for k in range(per):
            out.append(fn(bands[per * (l - 1) + 1 + k], betas[l - 1]))
    return out


def shrink(bands, beta, do_app=1):
    """x * s with s = 1 / (1 + beta) computed in the band's type; the approximation band only when `do_app`."""
    dt = bands[0].dtype.type
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = dt(dt(1) / (dt(1) + dt(beta)))
        out = [bands[0] * s if do_app else bands[0].copy()]
        out += [b * s for b in bands[1:]]
    return out


def group_soft(bands, levels, ndim, beta, do_app=0, normalize=0):
    """Per position, the detail bands of one level (and the approximation band at the last level when `do_app`) shrink by
    max(1 - beta / ||.||_2, 0), 0 where the norm is 0.  Computed in float64 for float32 bands and in np.longdouble for
    float64 bands, rounded once at the end.  Returns (bands, sumsq): sumsq[l - 1] is the wide sum of squares of level l, for
    callers that need to know where the band's own type would have under- or overflowed."""
    dt = bands[0].dtype.type
    wide = np.float64 if dt is np.float32 else np.longdouble
    per = per_level(ndim)
    betas = level_betas(beta, levels, normalize, dt)
    out = [b.copy() for b in bands]
    sumsq = []
    for l in range(1, levels + 1):
        idx = [per * (l - 1) + 1 + k for k in range(per)]
        if do_app and l == levels:
            idx.append(0)
        grp = [bands[i].astype(wide) for i in idx]
        ss = sum(g * g for g in grp)
        nrm = np.sqrt(ss)
        with np.errstate(divide="ignore", invalid="ignore"):
            res = np.where(nrm == 0, wide(0), np.fmax(wide(1) - wide(betas[l - 1]) / nrm, wide(0)))
        for i, g in zip(idx, grp):
            out[i] = (g * res).astype(dt)
        sumsq.append(ss)
    return out, sumsq


def axpy(dst, src, alpha):
    """dst + alpha * src in the next wider type, rounded once at the end (alpha is a `real_t` of the library)."""
    dt = dst[0].dtype.type
    wide = np.float64 if dt is np.float32 else np.longdouble
    a = wide(dt(alpha))
    return [(d.astype(wide) + a * s.astype(wide)).astype(dt) for d, s in zip(dst, src)]


def _fsum(a):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    step = 1 << 22
    return math.fsum(math.fsum(a[i:i + step].tolist()) for i in range(0, a.size, step)) if a.size > step else math.fsum(a.tolist())


def norms(bands):
    """(sum |c|, sum c^2) over all bands: exact sums (math.fsum) of float64 terms.  The squares of float32 values are exact in
    float64; those of float64 values are formed in np.longdouble and rounded to float64 once (2^-53 relative per term)."""
    n1 = math.fsum(_fsum(np.abs(b)) for b in bands)
    if bands[0].dtype == np.float32:
        n2 = math.fsum(_fsum(b.astype(np.float64) ** 2) for b in bands)
    else:
        n2 = math.fsum(_fsum((b.astype(np.longdouble) ** 2).astype(np.float64)) for b in bands)
    return n1, n2


def edge_vector(beta, dtype, ordinary=300, seed=5, finite_only=False):
    """The values a threshold kernel can get wrong: signed zeros, +-beta and its neighbours on both sides, the smallest and
    largest denormal, the smallest normal, +-max, +-inf, NaN, and `ordinary` values of a few beta around zero."""
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    b = dt(beta)
    inf = dt(np.inf)
    v = [dt(0.0), -dt(0.0), b, -b, np.nextafter(b, dt(0)), np.nextafter(-b, dt(0)), np.nextafter(b, inf), np.nextafter(-b, -inf),
         fi.smallest_subnormal, -fi.smallest_subnormal, np.nextafter(fi.tiny, dt(0)), -np.nextafter(fi.tiny, dt(0)),
         fi.tiny, -fi.tiny, fi.max, -fi.max]
    if not finite_only:
        v += [inf, -inf, dt(np.nan)]
    rng = np.random.default_rng(seed)
    v += list((rng.standard_normal(ordinary) * 3.0 * float(abs(b) if b != 0 else 1.0)).astype(dt))
    return np.array(v, dtype=dt)


def tile(vec, n):
    """`vec` repeated to length n."""
    reps = -(-n // vec.size)
    return np.tile(vec, reps)[:n].copy()


def same_bits(a, b):
    """Equal value for value, NaN where NaN, and the same sign on every zero."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))
