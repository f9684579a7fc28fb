"""Writes tests/golden/volume.npz: pywt.wavedecn(..., mode="periodization") of seeded float64 volumes, the reference that pins
the composition of tests/volume_ref.py (band naming, numbering, odd sizes) to PyWavelets.

Needs pywt (recorded with pywt 1.1.1, numpy 1.26 on Python 3.9); the tests read the .npz only.

    python tests/golden/make_volume_golden.py

Per case cK: cK_x the volume, cK_a the approximation, cK_l<level>_<key> the details, level 1 the FINEST (pywt lists the coarsest
first: level l is coeffs[levels + 1 - l]).
"""
import os

import numpy as np
import pywt

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, shape, wavelet, levels)
CASES = [("c0", (9, 10, 13), "db2", 1),
         ("c1", (7, 5, 6), "haar", 2),
         ("c2", (16, 12, 20), "sym4", 1),
         ("c3", (20, 24, 28), "db2", 2)]


def main():
    out = {"versions": np.array(["pywt " + pywt.__version__, "numpy " + np.__version__])}
    rng = np.random.default_rng(20250311)
    for name, shape, wname, lv in CASES:
        x = 300.0 * rng.standard_normal(shape)
        co = pywt.wavedecn(x, wname, mode="periodization", level=lv, axes=(0, 1, 2))
        assert len(co) == lv + 1
        out[name + "_x"] = x
        out[name + "_wname"] = np.array(wname)
        out[name + "_levels"] = np.int64(lv)
        out[name + "_a"] = np.ascontiguousarray(co[0], dtype=np.float64)
        for l in range(1, lv + 1):
            for key, band in sorted(co[lv + 1 - l].items()):
                out["%s_l%d_%s" % (name, l, key)] = np.ascontiguousarray(band, dtype=np.float64)
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, "volume.npz")
    np.savez_compressed(path, **out)
    print("wrote volume.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
