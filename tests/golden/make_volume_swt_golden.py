"""Writes tests/golden/volume_swt.npz: pywt.swtn of seeded float64 volumes and pywt.iswtn of random coefficients, the reference that
pins the composition of tests/volume_swt_ref.py (formulas, centres, the factor 1/2, band naming, numbering) to PyWavelets.

Needs pywt (recorded with pywt 1.1.1, numpy 1.26 on Python 3.9); the tests read the .npz only.

    python tests/golden/make_volume_swt_golden.py

Per case cK (c0 .. c3 are the four cases the transform was specified with; c4 is a small one with NON-integer data):
  cK_x            the volume: small integers (int8), to be read as float64; c4: float64 as drawn
  cK_fwd          pywt.swtn(x): the bands in `num` order -- A_L, then level 1 (the FINEST; pywt lists the coarsest first) aad .. ddd,
                  level 2 ... -- stacked, [1 + 7 L][Nz][Nr][Nc]
  cK_coef         random coefficients in the same order and shape: small integers (int8); c4: float64 as drawn
  cK_inv          pywt.iswtn of them, [Nz][Nr][Nc]

To keep the file below 300 KB the float64 results are stored in FIXED POINT: int64 = rint(value * 2^42).  Every value is below
2^8 in magnitude here, so the high bytes compress away; the rounding is at most 2^-43 = 1.2e-13, an eighth of the 1e-12 the
tests compare at -- which leaves the composition 8.8e-13 of the 1e-12, not all of it.  The integer inputs of c0 .. c3 are exact in
both programs, so they cost nothing; c4 (192 samples, stored as raw float64) is there so that ordinary real-valued data goes through
the same comparison.  tests/test_volume_swt_ref_cpu.py: golden().
"""
import os

import numpy as np
import pywt

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")
Q = 42

# (name, shape, wavelet, levels)
CASES = [("c0", (8, 8, 8), "haar", 3),
         ("c1", (8, 12, 16), "db2", 2),
         ("c2", (4, 8, 12), "db10", 1),
         ("c3", (6, 10, 4), "bior1.3", 1),
         ("c4", (4, 6, 8), "db2", 1)]
REAL_VALUED = ("c4",)


def fixed(a):
    a = np.asarray(a, dtype=np.float64)
    assert np.abs(a).max() < 2.0 ** 8
    return np.rint(a * 2.0 ** Q).astype(np.int64)


def main():
    out = {"versions": np.array(["pywt " + pywt.__version__, "numpy " + np.__version__]), "q": np.int64(Q)}
    rng = np.random.default_rng(20250617)
    for name, shape, wname, lv in CASES:
        real = name in REAL_VALUED
        x = 3.0 * rng.standard_normal(shape) if real else rng.integers(-8, 9, shape).astype(np.int8)
        co = pywt.swtn(x.astype(np.float64), wname, lv, axes=(0, 1, 2))
        assert len(co) == lv and all(sorted(d) == sorted(KEYS + ("aaa",)) for d in co)
        bands = [co[0]["aaa"]] + [co[lv - l][k] for l in range(1, lv + 1) for k in KEYS]
        coef = 7.0 * rng.standard_normal((1 + 7 * lv,) + shape) if real else rng.integers(-20, 21, (1 + 7 * lv,) + shape).astype(np.int8)
        # pywt.iswtn reads 'aaa' of the first (coarsest) dict only; the other dicts get one too, which must not matter
        dicts = []
        for l in range(lv, 0, -1):
            d = {k: coef[1 + 7 * (l - 1) + i].astype(np.float64) for i, k in enumerate(KEYS)}
            d["aaa"] = coef[0].astype(np.float64) if l == lv else rng.standard_normal(shape)
            dicts.append(d)
        y = pywt.iswtn(dicts, wname, axes=(0, 1, 2))
        out[name + "_x"] = x
        out[name + "_wname"] = np.array(wname)
        out[name + "_levels"] = np.int64(lv)
        out[name + "_fwd"] = fixed(np.stack(bands))
        out[name + "_coef"] = coef
        out[name + "_inv"] = fixed(y)
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, "volume_swt.npz")
    np.savez_compressed(path, **out)
    print("wrote volume_swt.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
