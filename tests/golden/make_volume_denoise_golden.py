"""Writes tests/golden/volume_denoise.npz: pywt.wavedecn(..., mode="periodization") of seeded noisy float64 volumes, with what
skimage.restoration's own helpers give for the sub-bands (noise estimate from the finest 'ddd' sub-band, universal and BayesShrink
thresholds), pywt.threshold of every sub-band in both modes with its BayesShrink threshold, and, for the even-sized volumes,
pywt.waverecn of the result: what pins tests/volume_ops_ref.py to PyWavelets and scikit-image.

Needs pywt and skimage (recorded with pywt 1.1.1, skimage 0.18.3, numpy 1.26 on Python 3.9); the tests read the .npz only.

    python tests/golden/make_volume_denoise_golden.py

Per case cK: cK_a the approximation, cK_l<level>_<key> the details, level 1 the FINEST (pywt lists the coarsest first);
cK_sigma, cK_visu, cK_bayes[7 L] in `num` order (num - 1); cK_<mode>_<num> the thresholded detail sub-bands; cK_rec_<mode> the
reconstruction (even-sized cases).
"""
import os

import numpy as np
import pywt
from skimage.restoration import _denoise as sk

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, shape, wavelet, levels)
CASES = [("c0", (12, 10, 14), "db2", 1),
         ("c1", (16, 16, 16), "haar", 2),
         ("c2", (20, 24, 28), "sym4", 2),
         ("c3", (9, 10, 13), "db2", 1)]
KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")
NOISE = 20.0


def pattern(shape):
    z, y, x = np.meshgrid(*[np.arange(n) / float(n) for n in shape], indexing="ij")
    return 128.0 + 80.0 * np.sin(2 * np.pi * z) * np.cos(2 * np.pi * y) + 40.0 * np.cos(4 * np.pi * x) * np.sin(2 * np.pi * y)


def main():
    out = {"versions": np.array(["pywt " + pywt.__version__, "skimage " + sk.__name__.split(".")[0] + " " + __import__("skimage").__version__,
                                 "numpy " + np.__version__])}
    rng = np.random.default_rng(20251019)
    for name, shape, wname, lv in CASES:
        x = pattern(shape) + NOISE * rng.standard_normal(shape)
        co = pywt.wavedecn(x, wname, mode="periodization", level=lv, axes=(0, 1, 2))
        assert len(co) == lv + 1
        sigma = sk._sigma_est_dwt(co[-1]["ddd"], distribution="Gaussian")
        out[name + "_wname"] = np.array(wname)
        out[name + "_levels"] = np.int64(lv)
        out[name + "_shape"] = np.array(shape, dtype=np.int64)
        out[name + "_a"] = np.ascontiguousarray(co[0], dtype=np.float64)
        out[name + "_sigma"] = np.float64(sigma)
        out[name + "_visu"] = np.float64(sk._universal_thresh(x, sigma))
        bayes = []
        thr = {"soft": [co[0]] + [dict() for _ in range(lv)], "hard": [co[0]] + [dict() for _ in range(lv)]}
        for l in range(1, lv + 1):
            for k, key in enumerate(KEYS):
                band = co[lv + 1 - l][key]
                out["%s_l%d_%s" % (name, l, key)] = np.ascontiguousarray(band, dtype=np.float64)
                t = sk._bayes_thresh(band, sigma ** 2)
                bayes.append(t)
                for mode in ("soft", "hard"):
                    res = pywt.threshold(band, value=t, mode=mode)
                    thr[mode][lv + 1 - l][key] = res
                    out["%s_%s_%d" % (name, mode, 1 + 7 * (l - 1) + k)] = np.ascontiguousarray(res, dtype=np.float64)
        out[name + "_bayes"] = np.array(bayes, dtype=np.float64)
        if all(n % (1 << lv) == 0 for n in shape):
            for mode in ("soft", "hard"):
                out["%s_rec_%s" % (name, mode)] = pywt.waverecn(thr[mode], wname, mode="periodization", axes=(0, 1, 2))
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, "volume_denoise.npz")
    np.savez_compressed(path, **out)
    print("wrote volume_denoise.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
