"""The rule a denoise table of the device is held to (tests/test_gpu_adaptive.py, tests/test_gpu_sequences.py): plain numpy, no GPU."""
import numpy as np

import adaptive_ref


def _id(p):
    return "-".join(str(x).replace(" ", "") for x in p)


def swept(band):
    """the swept length of a band: all its images, padded to 64 values"""
    return -(-band.size // 64) * 64


def check_table(p, bands, sigma, got_T, method, ref_stats=None):
    """The device's table against the reference's: the final rounding (2^-24, 2^-53 in fp64) plus A n 2^-52, A = m / |m - var| the
    cancellation factor, m the reference's mean(c^2), n the element count.  A (band, image) whose |m - var - eps| is below the
    band's sum bound may sit on either side of the max(., eps) and is left out; at most ONE per case."""
    dt = np.dtype(p.dtype)
    stats = adaptive_ref.band_stats(bands) if ref_stats is None else ref_stats
    want_T = adaptive_ref.threshold_table(bands, sigma, method, p.nsamples, stats=stats)
    assert np.all(np.isnan(got_T[0])) and got_T.dtype == dt and got_T.shape == (p.nbands, p.batch)
    rounding = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    eps = float(np.finfo(dt).eps)
    left_out, worst = 0, 0.0
    for b in range(1, p.nbands):
        n = bands[b][0].size
        for i in range(p.batch):
            g, r = float(got_T[b, i]), float(want_T[b, i])
            if method == "VisuShrink":
                assert abs(g - r) <= 2 * rounding * abs(r), (b, i, g, r)
                continue
            var = sigma[i] * sigma[i]
            m = stats[b, i, 1] / n
            if abs(m - var - eps) < 2.0 * swept(bands[b]) * 2.0 ** -53 * m:
                left_out += 1
                continue
            A = m / abs(m - var)
            bound = rounding + A * n * 2.0 ** -52
            worst = max(worst, abs(g - r) / abs(r) / bound)
            assert abs(g - r) <= bound * abs(r), (b, i, g, r, A, n)
    assert left_out <= 1, left_out
    print("denoise table %s %s %s: worst %.3g of the bound, %d left out" % (_id(p.spec), dt.name, method, worst, left_out))
    return want_T


def left_out_pairs(dtype, bands, sigma, method, stats):
    """How many (band, image) pairs check_table leaves out of one table: its condition, counted."""
    if method == "VisuShrink":
        return 0
    eps = float(np.finfo(np.dtype(dtype)).eps)
    count = 0
    for b in range(1, len(bands)):
        n = bands[b][0].size
        for i in range(bands[b].shape[0]):
            m = stats[b, i, 1] / n
            count += bool(abs(m - sigma[i] * sigma[i] - eps) < 2.0 * swept(bands[b]) * 2.0 ** -53 * m)
    return count
