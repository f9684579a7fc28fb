"""The 3D DWT of a volume [Nz][Nr][Nc] and its inverse as a COMPOSITION of the committed CPU oracle: one level is a one-level
1D oracle transform along the depth axis (moved last), then a one-level 2D oracle transform of every low and high slice.
Boundary rule of the oracle (odd lengths repeat their last sample, then periodic: pywt's "periodization").

Also here: the band naming and numbering of pdwt_volume (include/pypwt_amd.h), the level clamp, and the thresholds applied band
by band through tests/ops_ref.py.

`double`: False -- fp32 data and arithmetic; True -- fp32 data, fp64 accumulation (the stack between the depth step and the 2D step
stays fp32, as it does on the device); "full" -- fp64 data and arithmetic (the checker of the fp64 library, and the reference the
fp32 results are compared with).

`filt` = (hlen, dec_lo, dec_hi, rec_lo, rec_hi) replaces the named wavelet's bank on all three axes (tests/tap_banks.py);
`depth_filt` is a bank for the depth step alone (tests/test_volume_taps_cpu.py zeroes single taps there).  With both None
`wname` decides, as before.
"""
import numpy as np

import ops_ref
from oracle import oracle

# pywt.wavedecn's keys with axes (z, y, x) in sorted order -> (depth half, band of the 2D level: 0 A, 1 H, 2 V, 3 D)
KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")
SUB = {"aaa": (0, 0), "aad": (0, 2), "ada": (0, 1), "add": (0, 3), "daa": (1, 0), "dad": (1, 2), "dda": (1, 1), "ddd": (1, 3)}


def div2(n):
    return (n + (n & 1)) // 2


def ilog2(i):
    l = 0
    while i > 1:
        i >>= 1
        l += 1
    return l


def clamp_levels(shape, hlen, levels):
    """The reference's rule (wt.cu:155-165) on the smallest size; below one level: one, as pdwt_create does."""
    levels = max(int(levels), 1)
    return min(levels, max(ilog2(min(shape) // (hlen - 1)), 1))


def hlen_of(wname):
    return oracle.filters(wname)[0]


def _dtype(double):
    return np.float64 if double == "full" else np.float32


def _bank(filt, dt):
    """The oracle reads a bank's taps in the data's type."""
    return None if filt is None else (int(filt[0]),) + tuple(np.ascontiguousarray(t, dtype=dt) for t in filt[1:5])


def level_shapes(shape, levels):
    """[(depth, rows, cols)] of A_0 .. A_levels."""
    out = [tuple(shape)]
    for _ in range(levels):
        out.append(tuple(div2(n) for n in out[-1]))
    return out


def band_shapes(shape, levels):
    """(depth, rows, cols) of every coefficient index `num`: 0 = A_L, 1 + 7 (l - 1) + k, level 1 the finest."""
    ls = level_shapes(shape, levels)
    return [ls[levels]] + [ls[l] for l in range(1, levels + 1) for _ in KEYS]


def num_of(level, key):
    return 1 + 7 * (level - 1) + KEYS.index(key)


def forward_level(a, wname, double="full", filt=None, depth_filt=None):
    """One level: {key: band} with all eight keys ('aaa' is the approximation)."""
    dt = _dtype(double)
    filt = _bank(filt, dt)
    depth_filt = filt if depth_filt is None else _bank(depth_filt, dt)
    a = np.ascontiguousarray(a, dtype=dt)
    nz, nr, nc = a.shape
    # depth: one 1D level over the rows of [Nr * Nc][Nz]
    t = np.ascontiguousarray(np.moveaxis(a, 0, -1).reshape(nr * nc, nz))
    lo, hi = oracle.forward(t, wname, 1, ndim=1, double=double, filt=depth_filt)
    nz2 = div2(nz)
    halves = [np.moveaxis(np.asarray(h).reshape(nr, nc, nz2), -1, 0) for h in (lo, hi)]
    out = {k: np.empty((nz2, div2(nr), div2(nc)), dtype=dt) for k in SUB}
    for half, stack in enumerate(halves):
        for z in range(nz2):
            planes = oracle.forward(np.ascontiguousarray(stack[z]), wname, 1, ndim=2, double=double, filt=filt)
            for key, (h, b) in SUB.items():
                if h == half:
                    out[key][z] = planes[b]
    return out


def inverse_level(bands, shape, wname, double="full", filt=None, depth_filt=None):
    """{key: band} with all eight keys -> the volume of `shape` one level up."""
    dt = _dtype(double)
    filt = _bank(filt, dt)
    depth_filt = filt if depth_filt is None else _bank(depth_filt, dt)
    nz, nr, nc = shape
    nz2 = div2(nz)
    halves = []
    for half in (0, 1):
        stack = np.empty((nz2, nr, nc), dtype=dt)
        keys = [None] * 4
        for key, (h, b) in SUB.items():
            if h == half:
                keys[b] = key
        for z in range(nz2):
            stack[z] = oracle.inverse([np.ascontiguousarray(bands[k][z], dtype=dt) for k in keys], (nr, nc), wname, 1, ndim=2, double=double,
                                      filt=filt)
        halves.append(np.ascontiguousarray(np.moveaxis(stack, 0, -1).reshape(nr * nc, nz2)))
    t = oracle.inverse(halves, (nr * nc, nz), wname, 1, ndim=1, double=double, filt=depth_filt)
    return np.ascontiguousarray(np.moveaxis(np.asarray(t).reshape(nr, nc, nz), -1, 0))


def forward(vol, wname, levels, double="full", filt=None, depth_filt=None):
    """Bands in `num` order: [A_L, aad_1, ada_1, ..., ddd_1, aad_2, ...]; `levels` is taken as given (clamp_levels is the caller's)."""
    a = np.ascontiguousarray(vol, dtype=_dtype(double))
    details = []
    for _ in range(levels):
        lv = forward_level(a, wname, double, filt, depth_filt)
        details += [lv[k] for k in KEYS]
        a = lv["aaa"]
    return [a] + details


def inverse(bands, shape, wname, levels, double="full", filt=None, depth_filt=None):
    ls = level_shapes(shape, levels)
    a = np.asarray(bands[0])
    for l in range(levels, 0, -1):
        lv = {k: bands[num_of(l, k)] for k in KEYS}
        lv["aaa"] = a
        a = inverse_level(lv, ls[l - 1], wname, double, filt, depth_filt)
    return a


def to_wavedecn(bands, levels):
    """[A, {key: band} of the COARSEST level, ..., of level 1]: pywt.wavedecn's order."""
    return [bands[0]] + [{k: bands[num_of(l, k)] for k in KEYS} for l in range(levels, 0, -1)]


def threshold(bands, levels, op, beta, do_app=0, normalize=0):
    """soft / hard on every detail band, and on A_L when `do_app`, with the per-level betas of tests/ops_ref.py (level l:
    beta / sqrt(2)^l under `normalize`, the approximation beta / sqrt(2)^L): band by band, bit for bit the 2D plans' arithmetic."""
    dt = bands[0].dtype.type
    fn = {"soft": ops_ref.soft, "hard": ops_ref.hard}[op]
    betas = ops_ref.level_betas(beta, levels, normalize, dt)
    out = [fn(bands[0], ops_ref.app_beta(beta, levels, normalize, dt)) if do_app else bands[0].copy()]
    for l in range(1, levels + 1):
        out += [fn(bands[num_of(l, k)], betas[l - 1]) for k in KEYS]
    return out
