"""tests/volume_ops_ref.py pinned to recorded results of pywt and skimage.restoration's helpers on noisy volumes
(tests/golden/volume_denoise.npz, written by tests/golden/make_volume_denoise_golden.py), and the new pdwt_volume_* entry points
checked without a GPU: declared, exported by both libraries, and PDWT_ERR_ARG for a null handle.

  sigma, universal threshold   bit for bit
  BayesShrink thresholds       the summation bound (32 A + 4) 2^-53 that tests/test_adaptive_ref_cpu.py derives (A = m / |m - var|;
                               the largest sub-band here has 1680 values, below the 2^14 the derivation allows for)
  thresholded sub-bands, and the reconstruction of them through tests/volume_ref.py     1e-12 max(max|ref|, 1)
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ops_ref
import volume_ops_ref as ref
import volume_ref
from golden_util import GOLDEN

NEW_SYMBOLS = ["pdwt_volume_band_stats_async", "pdwt_volume_estimate_sigma_async", "pdwt_volume_threshold_bands", "pdwt_volume_denoise_async",
               "pdwt_volume_adaptive_slots", "pdwt_volume_select_magnitude_async", "pdwt_volume_keep_largest_async",
               "pdwt_volume_sparsify_slots", "pdwt_volume_norms_async", "pdwt_volume_read"]
WANT = {"c0": ((12, 10, 14), "db2", 1), "c1": ((16, 16, 16), "haar", 2), "c2": ((20, 24, 28), "sym4", 2), "c3": ((9, 10, 13), "db2", 1)}
PATH = os.path.join(GOLDEN, "volume_denoise.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(PATH)
    cases = []
    for name in z["cases"]:
        name = str(name)
        lv = int(z[name + "_levels"])
        bands = [z[name + "_a"]] + [z["%s_l%d_%s" % (name, l, k)] for l in range(1, lv + 1) for k in volume_ref.KEYS]
        c = dict(name=name, shape=tuple(int(n) for n in z[name + "_shape"]), wname=str(z[name + "_wname"]), levels=lv, bands=bands,
                 sigma=float(z[name + "_sigma"]), visu=float(z[name + "_visu"]), bayes=z[name + "_bayes"])
        for mode in ("soft", "hard"):
            c[mode] = [z["%s_%s_%d" % (name, mode, num)] for num in range(1, 1 + 7 * lv)]
            c["rec_" + mode] = z["%s_rec_%s" % (name, mode)] if "%s_rec_%s" % (name, mode) in z.files else None
        cases.append(c)
    return cases


def test_golden_file_is_what_the_generator_describes(golden):
    assert [c["name"] for c in golden] == sorted(WANT)
    for c in golden:
        shape, w, lv = WANT[c["name"]]
        assert (c["shape"], c["wname"], c["levels"]) == (shape, w, lv)
        assert [b.shape for b in c["bands"]] == volume_ref.band_shapes(shape, lv) and all(b.dtype == np.float64 for b in c["bands"])
        assert (c["rec_soft"] is not None) == all(n % (1 << lv) == 0 for n in shape)
        assert max(b.size for b in c["bands"]) <= 1 << 14
    assert os.path.getsize(PATH) < 512 * 1024


def test_sigma_is_skimage_s_bit_for_bit(golden):
    for c in golden:
        assert ref.estimate_sigma(c["bands"])[0] == c["sigma"], c["name"]
        assert ref.NOISE_BAND == volume_ref.num_of(1, "ddd")


def test_universal_threshold_is_skimage_s_bit_for_bit(golden):
    for c in golden:
        T = ref.threshold_table(c["bands"], c["sigma"], "VisuShrink", c["shape"])
        assert T.shape == (1 + 7 * c["levels"],) and np.isnan(T[0]) and np.all(T[1:] == c["visu"]), c["name"]


def test_bayes_thresholds_within_the_summation_bound(golden):
    worst = 0.0
    for c in golden:
        T = ref.threshold_table(c["bands"], c["sigma"], "BayesShrink", c["shape"])
        var = c["sigma"] ** 2
        for num in range(1, len(c["bands"])):
            d = c["bands"][num]
            m = ops_ref.norms([d])[1] / d.size
            want, got = float(c["bayes"][num - 1]), float(T[num])
            if m - var <= np.finfo(np.float64).eps:
                assert got == want == var / math.sqrt(np.finfo(np.float64).eps), (c["name"], num)
                continue
            A = m / abs(m - var)
            rel = abs(got - want) / abs(want)
            worst = max(worst, rel / 2.0 ** -53)
            assert rel <= (32 * A + 4) * 2.0 ** -53, (c["name"], num, rel, A)
    print("worst BayesShrink difference: %.2f * 2^-53" % worst)


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_thresholded_sub_bands_and_their_reconstruction(golden, mode):
    for c in golden:
        table = np.concatenate([[np.nan], c["bayes"]])
        out = ref.threshold_bands(c["bands"], table, mode)
        assert np.array_equal(out[0], c["bands"][0])
        for num in range(1, len(out)):
            want = c[mode][num - 1]
            tol = 1e-12 * max(float(np.abs(want).max()), 1.0)
            assert out[num].shape == want.shape and float(np.abs(out[num] - want).max()) <= tol, (c["name"], num)
        if c["rec_" + mode] is not None:
            rec = volume_ref.inverse(out, c["shape"], c["wname"], c["levels"], "full")
            want = c["rec_" + mode]
            assert float(np.abs(rec - want).max()) <= 1e-12 * max(float(np.abs(want).max()), 1.0), c["name"]
        # the whole recipe gives the same table and the same sweep
        sigma, T, den = ref.denoise(c["bands"], c["shape"], "BayesShrink", mode)
        assert sigma[0] == c["sigma"] and np.array_equal(T, ref.threshold_table(c["bands"], c["sigma"], "BayesShrink", c["shape"]), equal_nan=True)
        assert all(np.array_equal(a, b) for a, b in zip(den, ref.threshold_bands(c["bands"], T, mode)))


def test_sums_and_k_term_pair_on_sub_bands(golden):
    c = golden[3]
    st = ref.band_stats(c["bands"])
    assert st.shape == (8, 2) and st[7, 1] == ops_ref.norms([c["bands"][7]])[1]
    n = ref.count(c["bands"])
    assert n == sum(b.size for b in c["bands"][1:]) and ref.count(c["bands"], 1) == n + c["bands"][0].size
    thr, kept, out = ref.keep_largest(c["bands"], n // 4)
    mags = np.sort(np.abs(np.concatenate([b.ravel() for b in c["bands"][1:]])))
    assert thr[0] == mags[n - n // 4] and kept[0] == n // 4 == sum(int(np.count_nonzero(b)) for b in out[1:])
    assert np.array_equal(out[0], c["bands"][0]) and [b.shape for b in out] == [b.shape for b in c["bands"]]
    assert np.array_equal(ref.select_magnitude(c["bands"], n // 4)[0], thr)


# ------------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_header_declares_the_new_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "pypwt_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in txt, name
    scope = txt[txt.index("Out of scope: 3D SWT"):txt.index("typedef struct pdwt_volume* pdwt_volume_handle;")]
    assert "K-term" not in scope and "adaptive" not in scope


@pytest.mark.parametrize("variant", ["f32", "f64"])
def test_both_libraries_export_them_and_refuse_a_null_handle(variant):
    from pypwt_amd.build import build_library
    build_library(verbose=False, variant=variant)
    from pypwt_amd import _lib
    lib = _lib.load(variant)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), (variant, name)
        assert name in _lib.SIGNATURES
    table = (lib.pdwt_real * 8)()
    sigma = (C.c_double * 1)(1.0)
    slot = C.c_void_p()
    buf = (C.c_double * 2)()
    assert lib.pdwt_volume_band_stats_async(None, None) == _lib.ERR_ARG
    assert lib.pdwt_volume_estimate_sigma_async(None, 1, None) == _lib.ERR_ARG
    assert lib.pdwt_volume_threshold_bands(None, 0, table, 0) == _lib.ERR_ARG
    assert lib.pdwt_volume_denoise_async(None, 0, 0, sigma, 1) == _lib.ERR_ARG
    assert lib.pdwt_volume_denoise_async(None, 0, 0, None, 1) == _lib.ERR_ARG
    assert lib.pdwt_volume_adaptive_slots(None, C.byref(slot), None, None) == _lib.ERR_ARG
    assert lib.pdwt_volume_select_magnitude_async(None, 3, 0, None, None) == _lib.ERR_ARG
    assert lib.pdwt_volume_keep_largest_async(None, 3, 0) == _lib.ERR_ARG
    assert lib.pdwt_volume_sparsify_slots(None, C.byref(slot), None) == _lib.ERR_ARG
    assert lib.pdwt_volume_norms_async(None, None) == _lib.ERR_ARG
    assert lib.pdwt_volume_read(None, buf, buf, 16) == _lib.ERR_ARG
    assert b"null volume handle" in lib.pdwt_last_error() or b"bad arguments" in lib.pdwt_last_error()
    assert not slot.value


def test_python_classes_have_the_new_methods_with_wavelets_signatures():
    import inspect
    from pypwt_amd import Wavelets, Wavelets3D, Wavelets3D64
    assert issubclass(Wavelets3D64, Wavelets3D)
    for m in ("band_stats", "read_band_stats", "estimate_sigma", "read_sigma", "threshold_bands", "denoise", "last_thresholds",
              "select_magnitude", "keep_largest", "last_sparsify", "norms_device", "read_norms"):
        got = inspect.signature(getattr(Wavelets3D, m)).parameters
        want = inspect.signature(getattr(Wavelets, m)).parameters
        assert [(k, v.default) for k, v in got.items()] == [(k, v.default) for k, v in want.items()], m
        assert getattr(Wavelets3D64, m) is getattr(Wavelets3D, m)
