"""Writes tests/golden/adaptive.npz: float64 detail bands of pywt transforms of a smooth pattern plus Gaussian noise, with what
skimage.restoration's own helpers give for them (noise estimate, BayesShrink and universal thresholds).

Needs pywt and skimage (recorded with pywt 1.1.1, skimage 0.18.3, numpy 1.26 on Python 3.9); the tests read the .npz only.

    python tests/golden/make_adaptive_golden.py
"""
import os

import numpy as np
import pywt
from skimage.restoration import _denoise as sk

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, shape, wavelet, levels, noise sigma, pattern amplitude)
CASES = [("c0", (256, 256), "db4", 3, 10.0, 100.0),
         ("c1", (120, 200), "sym8", 2, 25.0, 60.0),
         ("c2", (64, 64), "haar", 4, 3.0, 200.0),
         ("c3", (1, 4096), "db2", 5, 1.0, 20.0),
         ("c4", (96, 96), "db2", 3, 40.0, 5.0)]


def pattern(shape, amp):
    r, c = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return amp * (np.sin(2 * np.pi * c / 97.0) * np.cos(2 * np.pi * r / 61.0) + 0.5 * ((c // 32 + r // 32) % 2))


def main():
    out = {}
    rng = np.random.default_rng(20240607)
    for name, shape, wname, lv, sig, amp in CASES:
        x = pattern(shape, amp) + sig * rng.standard_normal(shape)
        if shape[0] == 1:
            co = pywt.wavedec(x[0], wname, mode="periodization", level=lv)
            details = [d for d in co[1:]][::-1]          # finest first: D1, D2, ...
            noise = details[0]
        else:
            co = pywt.wavedec2(x, wname, mode="periodization", level=lv)
            details = [b for lvl in co[1:][::-1] for b in lvl]   # H1, V1, D1, H2, ...
            noise = details[2]
        sigma = sk._sigma_est_dwt(noise, distribution="Gaussian")
        var = sigma ** 2
        out[name + "_n"] = np.int64(len(details))
        out[name + "_size"] = np.int64(x.size)
        out[name + "_ndim"] = np.int64(1 if shape[0] == 1 else 2)
        out[name + "_sigma"] = np.float64(sigma)
        out[name + "_visu"] = np.float64(sk._universal_thresh(x, sigma))
        out[name + "_bayes"] = np.array([sk._bayes_thresh(d, var) for d in details], dtype=np.float64)
        for k, d in enumerate(details):
            out["%s_d%d" % (name, k)] = np.ascontiguousarray(d, dtype=np.float64)
    out["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(os.path.join(HERE, "adaptive.npz"), **out)
    print("wrote adaptive.npz", os.path.getsize(os.path.join(HERE, "adaptive.npz")), "bytes")


if __name__ == "__main__":
    main()
