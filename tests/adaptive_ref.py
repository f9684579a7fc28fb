"""Plain numpy restatement of the adaptive denoising operators (band_stats, estimate_sigma, threshold_bands, denoise).

Bands come in the plan's order (band 0 = approximation, then the detail bands level by level) and every band is an array
whose LEADING axis is the image of the batch: (batch, rows, cols); `images()` makes that shape out of what the classes
return.  The rows of a batched-1D plan are pooled: such a band is (1, rows, cols).

  median   np.sort of |c| with the zeros removed, the two middle elements averaged in double
  sums     math.fsum of float64 terms, as ops_ref.norms
  BayesShrink  T = var / sqrt(max(mean(c^2) - var, eps)), var = sigma^2, in double, rounded once to the band's type
  VisuShrink   T = sigma sqrt(2 ln N), N = samples of the image
  sweep    ops_ref.soft / ops_ref.hard per (band, image); a NaN threshold leaves that band of that image as it is

tests/test_adaptive_ref_cpu.py pins the median and the two formulas to recorded results of skimage.restoration's helpers.
"""
import math

import numpy as np

import ops_ref

SIGMA_DENOMINATOR = 0.6744897501960817  # scipy.stats.norm.ppf(0.75)


def images(band, batch):
    """(batch, rows, cols) view of a band as the classes return it: (rows, cols) from Wavelets, (batch, rows, cols) from
    BatchedWavelets."""
    band = np.asarray(band)
    return band.reshape((batch, -1, band.shape[-1]))


def noise_band(ndim):
    """`num` of the band the noise is estimated from: the finest diagonal band in 2D, the finest detail band in 1D."""
    return 3 if ndim == 2 else 1


def median_abs(x, skip_zeros=True):
    """Exact median of |x| as a float64: the middle element of the sorted magnitudes, or the mean in double of the two middle
    elements; exact zeros (and -0.0) are left out when `skip_zeros`; NaNs sort last; nothing left gives 0."""
    a = np.abs(np.asarray(x).ravel())
    if skip_zeros:
        a = a[a != 0]
    if a.size == 0:
        return 0.0
    s = np.sort(a)
    n = s.size
    if n % 2:
        return float(s[n // 2])
    lo, hi = float(s[n // 2 - 1]), float(s[n // 2])
    return lo if lo == hi else (lo + hi) * 0.5


def estimate_sigma(band, skip_zeros=True):
    """sigma per image of one (batch, rows, cols) band: median(|c|) / 0.6745."""
    return np.array([median_abs(img, skip_zeros) / SIGMA_DENOMINATOR for img in band], dtype=np.float64)


def band_stats(bands):
    """[nbands][batch][2] float64: (sum |c|, sum c^2) of every image of every band, exact sums of float64 terms."""
    out = np.zeros((len(bands), bands[0].shape[0], 2), dtype=np.float64)
    for b, band in enumerate(bands):
        for i, img in enumerate(band):
            out[b, i] = ops_ref.norms([img])
    return out


def bayes_threshold(sumsq, n, sigma, dtype):
    """BayesShrink threshold of one (band, image) from its sum of squares, in double, rounded once to `dtype`."""
    var = np.float64(sigma) * np.float64(sigma)
    m = np.float64(sumsq) / np.float64(n)
    eps = np.float64(np.finfo(dtype).eps)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.dtype(dtype).type(var / np.sqrt(max(m - var, eps)))


def visu_threshold(sigma, nsamples, dtype):
    """The universal threshold sigma sqrt(2 ln N), in double, rounded once to `dtype`."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.dtype(dtype).type(np.float64(sigma) * math.sqrt(2.0 * math.log(nsamples)))


def threshold_table(bands, sigma, method, nsamples, stats=None):
    """[nbands][batch] thresholds in the bands' type; row 0 (the approximation) is NaN."""
    dt = bands[0].dtype
    batch = bands[0].shape[0]
    if stats is None:
        stats = band_stats(bands)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (batch,))
    T = np.full((len(bands), batch), np.nan, dtype=dt)
    for b in range(1, len(bands)):
        n = bands[b][0].size
        for i in range(batch):
            if method == "BayesShrink":
                T[b, i] = bayes_threshold(stats[b, i, 1], n, sigma[i], dt)
            elif method == "VisuShrink":
                T[b, i] = visu_threshold(sigma[i], nsamples, dt)
            else:
                raise ValueError(method)
    return T


def threshold_bands(bands, table, op="soft"):
    """soft / hard per (band, image) with table[band][image]; NaN entries leave that band of that image untouched."""
    fn = {"soft": ops_ref.soft, "hard": ops_ref.hard}[op]
    table = np.asarray(table)
    if table.ndim == 1:
        table = np.repeat(table[:, None], bands[0].shape[0], axis=1)
    out = []
    for b, band in enumerate(bands):
        res = band.copy()
        for i in range(band.shape[0]):
            t = table[b, i]
            if not np.isnan(t):
                res[i] = fn(band[i], t)
        out.append(res)
    return out


def denoise(bands, ndim, nsamples, method="BayesShrink", op="soft", sigma=None, skip_zeros=True):
    """The whole recipe: (sigma[batch], table[nbands][batch], thresholded bands)."""
    if sigma is None:
        sigma = estimate_sigma(bands[noise_band(ndim)], skip_zeros)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (bands[0].shape[0],)).copy()
    table = threshold_table(bands, sigma, method, nsamples)
    return sigma, table, threshold_bands(bands, table, op)
