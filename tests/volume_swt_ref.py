"""The STATIONARY 3D transform of a volume [Nz][Nr][Nc] and its inverse as a composition of per-axis a-trous steps in numpy:
the oracle's SWT formulas (oracle/pdwt_oracle.c:199-277) restated with np.roll on one axis at a time, axes in the order z, y, x.

    analysis   lo[g] = sum_j x[(g + (j - c) f) mod N] * dec_lo[hlen - 1 - j],  c = hlen / 2 - 1     (hi likewise with dec_hi)
    synthesis  out[g] = 1/2 sum_j (lo[(g + (j - c) f) mod N] * rec_lo[hlen - 1 - j] + hi[same] * rec_hi[hlen - 1 - j]),  c = hlen / 2

with f = 2^(level - 1).  tests/test_volume_swt_ref_cpu.py pins it to pywt.swtn / pywt.iswtn (tests/golden/volume_swt.npz) and its
y and x steps to the oracle's 2D SWT.  Any size from 1 on works (the index is a true modulo), odd sizes too, which pywt refuses.

Also here: band numbering and shapes of a stationary pdwt_volume (include/pypwt_amd.h) -- those of tests/volume_ref.py with every
band of the volume's own shape --, the level clamp, and the thresholds through tests/ops_ref.py.

`double`: "full" -- fp64 data and arithmetic; False -- fp32 data and arithmetic (every product and sum rounds to fp32; the stack
between the depth step and the 2D step is fp32, as on the device); True -- fp32 data and fp32 taps, every axis step accumulated in
fp64 and rounded to fp32 ONCE per step (so the volume between the depth step and the 2D steps is fp32 here too): the meaning
double=True has in tests/volume_ref.py, and the reference tests/tap_banks.py measures a correct fp32 evaluation's noise against.

`filt` = (hlen, dec_lo, dec_hi, rec_lo, rec_hi) replaces the named wavelet's bank on all three axes; `depth_filt` is a bank for
the depth step alone.
"""
import numpy as np

import ops_ref
from oracle import oracle
from volume_ref import KEYS, SUB, clamp_levels, hlen_of, num_of  # noqa: F401  (the numbering is the decimated volume's)


def _dtype(double):
    if not (isinstance(double, str) and double == "full") and double not in (False, True):
        raise ValueError("volume_swt_ref: double must be 'full', True or False")
    return np.float64 if double == "full" else np.float32


def _f64acc(double):
    return not isinstance(double, str) and bool(double)


def bank(wname, double, filt=None):
    """(hlen, dec_lo, dec_hi, rec_lo, rec_hi) with the taps in the data's type."""
    dt = _dtype(double)
    if filt is None:
        filt = oracle.filters(wname, dt)
    return (int(filt[0]),) + tuple(np.ascontiguousarray(t, dtype=dt) for t in filt[1:5])


def _f64acc_analysis(x, lo, hi, level, axis):
    """analysis_axis with every sum in fp64 -- the products of two fp32 values are exact there -- and ONE rounding to x's type."""
    hlen, f, c = len(lo), 1 << (level - 1), len(lo) // 2 - 1
    wide = x.astype(np.float64)
    aL, aH = np.zeros_like(wide), np.zeros_like(wide)
    for j in range(hlen):
        v = np.roll(wide, -(j - c) * f, axis=axis)
        aL = aL + v * np.float64(lo[hlen - 1 - j])
        aH = aH + v * np.float64(hi[hlen - 1 - j])
    return aL.astype(x.dtype), aH.astype(x.dtype)


def _f64acc_synthesis(a, d, rlo, rhi, level, axis):
    """synthesis_axis with every sum in fp64 (the halving is exact) and ONE rounding to a's type."""
    hlen, f, c = len(rlo), 1 << (level - 1), len(rlo) // 2
    wa, wd = a.astype(np.float64), d.astype(np.float64)
    ra, rd = np.zeros_like(wa), np.zeros_like(wd)
    for j in range(hlen):
        ra = ra + np.roll(wa, -(j - c) * f, axis=axis) * np.float64(rlo[hlen - 1 - j]) / 2.0
        rd = rd + np.roll(wd, -(j - c) * f, axis=axis) * np.float64(rhi[hlen - 1 - j]) / 2.0
    return (ra + rd).astype(a.dtype)


def analysis_axis(x, lo, hi, level, axis, f64acc=False):
    """One undecimated analysis step along `axis`: (low, high), both of x's shape and type; `f64acc`: summed in fp64, rounded once."""
    if f64acc:
        return _f64acc_analysis(x, lo, hi, level, axis)
    hlen, f, c = len(lo), 1 << (level - 1), len(lo) // 2 - 1
    dt = x.dtype.type
    aL, aH = np.zeros_like(x), np.zeros_like(x)
    for j in range(hlen):
        v = np.roll(x, -(j - c) * f, axis=axis)  # v[g] = x[(g + (j - c) f) mod N]
        aL = aL + v * dt(lo[hlen - 1 - j])
        aH = aH + v * dt(hi[hlen - 1 - j])
    return aL, aH


def synthesis_axis(a, d, rlo, rhi, level, axis, f64acc=False):
    """One undecimated synthesis step along `axis`; the factor 1/2 sits inside the sum (pdwt_oracle.c:253-254)."""
    if f64acc:
        return _f64acc_synthesis(a, d, rlo, rhi, level, axis)
    hlen, f, c = len(rlo), 1 << (level - 1), len(rlo) // 2
    dt = a.dtype.type
    ra, rd = np.zeros_like(a), np.zeros_like(d)
    for j in range(hlen):
        ra = ra + np.roll(a, -(j - c) * f, axis=axis) * dt(rlo[hlen - 1 - j]) / dt(2)
        rd = rd + np.roll(d, -(j - c) * f, axis=axis) * dt(rhi[hlen - 1 - j]) / dt(2)
    return ra + rd


def forward_level(a, level, filt, depth_filt=None, f64acc=False):
    """{key: band} with all eight keys of one level at dilation 2^(level - 1); key = (z, y, x) letters, 'a' low, 'd' high."""
    depth_filt = depth_filt or filt
    out = {"": a}
    for axis, fb in ((0, depth_filt), (1, filt), (2, filt)):
        nxt = {}
        for key, band in out.items():
            lo, hi = analysis_axis(band, fb[1], fb[2], level, axis, f64acc)
            nxt[key + "a"], nxt[key + "d"] = lo, hi
        out = nxt
    return out


def inverse_level(bands, level, filt, depth_filt=None, f64acc=False):
    """{key: band} with all eight keys -> the approximation one level up: x, then y (the device's 2D inverse), then z."""
    depth_filt = depth_filt or filt
    cur = dict(bands)
    for axis, fb in ((2, filt), (1, filt), (0, depth_filt)):
        nxt = {}
        for key in {k[:-1] for k in cur}:
            nxt[key] = synthesis_axis(cur[key + "a"], cur[key + "d"], fb[3], fb[4], level, axis, f64acc)
        cur = nxt
    return cur[""]


def forward(vol, wname, levels, double="full", filt=None, depth_filt=None):
    """Bands in `num` order: [A_L, aad_1, ..., ddd_1, aad_2, ...], level 1 the finest; `levels` is taken as given."""
    fb = bank(wname, double, filt)
    dfb = bank(wname, double, depth_filt) if depth_filt is not None else None
    a = np.ascontiguousarray(vol, dtype=_dtype(double))
    details = []
    for l in range(1, levels + 1):
        lv = forward_level(a, l, fb, dfb, _f64acc(double))
        details += [lv[k] for k in KEYS]
        a = lv["aaa"]
    return [a] + details


def inverse(bands, wname, levels, double="full", filt=None, depth_filt=None):
    fb = bank(wname, double, filt)
    dfb = bank(wname, double, depth_filt) if depth_filt is not None else None
    dt = _dtype(double)
    a = np.ascontiguousarray(bands[0], dtype=dt)
    for l in range(levels, 0, -1):
        lv = {k: np.ascontiguousarray(bands[num_of(l, k)], dtype=dt) for k in KEYS}
        lv["aaa"] = a
        a = inverse_level(lv, l, fb, dfb, _f64acc(double))
    return a


def forward_2d(img, wname, levels, double="full"):
    """The y and x steps alone on an image [Nr][Nc]: [A_L, H_1, V_1, D_1, H_2, ...] in the 2D plan's order (H = 'da': high along
    y; V = 'ad'; D = 'dd'), to be compared with oracle.forward(..., ndim=2, do_swt=1)."""
    fb = bank(wname, double)
    a = np.ascontiguousarray(img, dtype=_dtype(double))[None]
    out = []
    for l in range(1, levels + 1):
        lo, hi = analysis_axis(a, fb[1], fb[2], l, 2)  # rows first: along x
        A, H = analysis_axis(lo, fb[1], fb[2], l, 1)
        V, D = analysis_axis(hi, fb[1], fb[2], l, 1)
        out += [H[0], V[0], D[0]]
        a = A
    return [a[0]] + out


def inverse_2d(bands, wname, levels, double="full"):
    fb = bank(wname, double)
    dt = _dtype(double)
    a = np.ascontiguousarray(bands[0], dtype=dt)[None]
    for l in range(levels, 0, -1):
        H, V, D = (np.ascontiguousarray(bands[1 + 3 * (l - 1) + k], dtype=dt)[None] for k in range(3))
        lo = synthesis_axis(a, V, fb[3], fb[4], l, 2)  # along x first, as inverse_level does
        hi = synthesis_axis(H, D, fb[3], fb[4], l, 2)
        a = synthesis_axis(lo, hi, fb[3], fb[4], l, 1)
    return a[0]


def band_shapes(shape, levels):
    """(depth, rows, cols) of every coefficient index `num`: all of the volume's shape."""
    return [tuple(shape)] * (1 + 7 * levels)


def to_swtn(bands, levels):
    """pywt.swtn's list, coarsest level first, as far as a stationary volume keeps it: the first dict holds 'aaa' = A_L (the one
    pywt.iswtn reads); the 'aaa' of the finer levels are intermediates and are left out."""
    out = []
    for l in range(levels, 0, -1):
        d = {k: bands[num_of(l, k)] for k in KEYS}
        if l == levels:
            d["aaa"] = bands[0]
        out.append(d)
    return out


def threshold(bands, levels, op, beta, do_app=0, normalize=0):
    """soft / hard on every detail band, and on A_L when `do_app`, with the per-level betas of tests/ops_ref.py."""
    dt = bands[0].dtype.type
    fn = {"soft": ops_ref.soft, "hard": ops_ref.hard}[op]
    betas = ops_ref.level_betas(beta, levels, normalize, dt)
    out = [fn(bands[0], ops_ref.app_beta(beta, levels, normalize, dt)) if do_app else bands[0].copy()]
    for l in range(1, levels + 1):
        out += [fn(bands[num_of(l, k)], betas[l - 1]) for k in KEYS]
    return out
