"""Plain numpy restatement of the adaptive and K-term operators of a volume (`Wavelets3D.band_stats`, `estimate_sigma`,
`threshold_bands`, `denoise`, `select_magnitude`, `keep_largest`): thin, on top of tests/adaptive_ref.py and tests/sparsify_ref.py.

A volume is ONE image: its sub-bands, in `num` order (tests/volume_ref.py: 0 = A_L, then 1 + 7 (l - 1) + k), go into those two
as (1, depth * rows, cols) bands.  What differs from a 2D plan is only
  * the noise band: `num` 7, the finest 'ddd' sub-band (skimage.restoration.denoise_wavelet: dcoeffs[-1]['d' * ndim]);
  * VisuShrink's N: the size of the volume.
tests/test_volume_ops_ref_cpu.py pins this to recorded results of pywt and skimage (tests/golden/volume_denoise.npz).
"""
import numpy as np

import adaptive_ref
import sparsify_ref

NOISE_BAND = 7


def as_images(bands):
    """[(depth, rows, cols)] -> [(1, depth * rows, cols)]: every sub-band the one image of a band."""
    return [np.ascontiguousarray(b).reshape(1, b.shape[0] * b.shape[1], b.shape[2]) for b in bands]


def as_volumes(images, like):
    return [im.reshape(b.shape) for im, b in zip(images, like)]


def band_stats(bands):
    """(nbands, 2) float64: (sum |c|, sum c^2) of every sub-band, exact sums of float64 terms."""
    return adaptive_ref.band_stats(as_images(bands))[:, 0, :]


def estimate_sigma(bands, skip_zeros=True):
    """(1,) float64: median(|ddd_1|) / 0.6745 over the whole sub-band."""
    return adaptive_ref.estimate_sigma(as_images(bands)[NOISE_BAND], skip_zeros)


def threshold_table(bands, sigma, method, shape, stats=None):
    """(nbands,) thresholds in the bands' type, NaN at index 0; `shape`: the volume's."""
    if stats is not None:
        stats = np.asarray(stats).reshape(len(bands), 1, 2)
    return adaptive_ref.threshold_table(as_images(bands), sigma, method, int(np.prod(shape)), stats=stats)[:, 0]


def threshold_bands(bands, table, op="soft"):
    return as_volumes(adaptive_ref.threshold_bands(as_images(bands), np.asarray(table), op), bands)


def denoise(bands, shape, method="BayesShrink", op="soft", sigma=None, skip_zeros=True):
    """(sigma (1,), table (nbands,), the sub-bands after the sweep)."""
    if sigma is None:
        sigma = estimate_sigma(bands, skip_zeros)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (1,)).copy()
    table = threshold_table(bands, sigma, method, shape)
    return sigma, table, threshold_bands(bands, table, op)


def count(bands, do_app=0):
    """N: the elements of the swept sub-bands."""
    return sparsify_ref.count(as_images(bands), do_app)


def select_magnitude(bands, k, do_app=0):
    """(threshold (1,) in the bands' type, kept (1,) uint64)."""
    return sparsify_ref.select_magnitude(as_images(bands), k, do_app)


def keep_largest(bands, k, do_app=0):
    """(threshold (1,), kept (1,), the sub-bands after the sweep)."""
    thr, kept, out = sparsify_ref.keep_largest(as_images(bands), k, do_app)
    return thr, kept, as_volumes(out, bands)
