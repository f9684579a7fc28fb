"""tests/adaptive_ref.py pinned to recorded results of skimage.restoration's helpers (tests/golden/adaptive.npz, written by
tests/golden/make_adaptive_golden.py), and the new entry points of the C ABI checked without a GPU: declared, exported by
both libraries, and PDWT_ERR_ARG for a null handle."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import adaptive_ref
import ops_ref
from golden_util import GOLDEN

NEW_SYMBOLS = ["pdwt_band_stats_async", "pdwt_estimate_sigma_async", "pdwt_threshold_bands", "pdwt_denoise_async", "pdwt_adaptive_slots"]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "adaptive.npz"))
    cases = []
    for name in z["cases"]:
        name = str(name)
        details = [z["%s_d%d" % (name, k)] for k in range(int(z[name + "_n"]))]
        cases.append(dict(name=name, details=details, size=int(z[name + "_size"]), ndim=int(z[name + "_ndim"]),
                          sigma=float(z[name + "_sigma"]), visu=float(z[name + "_visu"]), bayes=z[name + "_bayes"]))
    assert len(cases) >= 5
    return cases


def _bands(case):
    """The recorded detail bands as the reference's band list: a dummy approximation, then (1, rows, cols) bands."""
    return [np.zeros((1, 1, 1))] + [np.atleast_2d(d)[None] for d in case["details"]]


def test_sigma_is_skimage_s_bit_for_bit(golden):
    for c in golden:
        noise = _bands(c)[adaptive_ref.noise_band(c["ndim"])]
        assert adaptive_ref.estimate_sigma(noise)[0] == c["sigma"], c["name"]


def test_universal_threshold_is_skimage_s_bit_for_bit(golden):
    for c in golden:
        assert adaptive_ref.visu_threshold(c["sigma"], c["size"], np.float64) == c["visu"], c["name"]
        T = adaptive_ref.threshold_table(_bands(c), c["sigma"], "VisuShrink", c["size"])
        assert np.isnan(T[0, 0]) and np.all(T[1:, 0] == c["visu"])


def test_bayes_thresholds_within_the_summation_bound(golden):
    """The only difference is how mean(c^2) is summed (np.mean pairwise against fsum): numpy sums blocks of 128 terms on 8
    accumulators and then pairwise, 16 + 3 + 7 roundings at most for the 2^14 terms of the largest band; the subtraction of
    var amplifies that by A = m / |m - var|; the division and the square root add a rounding each: (32 A + 4) 2^-53."""
    worst, eps_branch, near = 0.0, 0, 0
    for c in golden:
        bands = _bands(c)
        T = adaptive_ref.threshold_table(bands, c["sigma"], "BayesShrink", c["size"])
        var = c["sigma"] ** 2
        for k, d in enumerate(c["details"]):
            m = ops_ref.norms([d])[1] / d.size
            want, got = float(c["bayes"][k]), float(T[k + 1, 0])
            if m - var <= np.finfo(np.float64).eps:
                eps_branch += 1
                assert got == want == var / math.sqrt(np.finfo(np.float64).eps), (c["name"], k)
                continue
            A = m / abs(m - var)
            near += A > 50
            rel = abs(got - want) / abs(want)
            worst = max(worst, rel / 2.0 ** -53)
            assert rel <= (32 * A + 4) * 2.0 ** -53, (c["name"], k, rel, A)
    print("worst BayesShrink difference: %.2f * 2^-53; %d bands on the eps branch, %d with A > 50" % (worst, eps_branch, near))
    assert eps_branch >= 1  # the fixtures reach the max(., eps) branch


def test_sweep_and_recipe_are_consistent(golden):
    """threshold_bands applies ops_ref.soft / hard per (band, image), NaN leaves a pair alone, a (nbands,) table is one row
    for all images; denoise = estimate_sigma + threshold_table + threshold_bands."""
    c = golden[0]
    rng = np.random.default_rng(1)
    bands = [rng.standard_normal((3, 4, 5)).astype(np.float32) for _ in range(4)]
    table = np.array([[np.nan] * 3, [0.5, np.nan, 1.0], [0.1, 0.2, 0.3], [2.0, 0.0, -0.5]], dtype=np.float32)
    for op, fn in (("soft", ops_ref.soft), ("hard", ops_ref.hard)):
        out = adaptive_ref.threshold_bands(bands, table, op)
        for b in range(4):
            for i in range(3):
                want = bands[b][i] if np.isnan(table[b, i]) else fn(bands[b][i], table[b, i])
                assert ops_ref.same_bits(out[b][i], want)
    row = adaptive_ref.threshold_bands(bands, table[:, 0], "soft")
    full = adaptive_ref.threshold_bands(bands, np.repeat(table[:, :1], 3, axis=1), "soft")
    assert all(ops_ref.same_bits(a, b) for a, b in zip(row, full))
    bands = _bands(c)
    sigma, T, out = adaptive_ref.denoise(bands, c["ndim"], c["size"])
    assert sigma[0] == c["sigma"] and np.isnan(T[0, 0])
    assert all(ops_ref.same_bits(a, b) for a, b in zip(out, adaptive_ref.threshold_bands(bands, T, "soft")))
    st = adaptive_ref.band_stats(bands)
    assert st.shape == (len(bands), 1, 2) and st[1, 0, 1] == ops_ref.norms([bands[1]])[1]


def test_median_conventions():
    m = adaptive_ref.median_abs
    assert m(np.array([0.0, -0.0, 3.0, -1.0], dtype=np.float32)) == 2.0
    assert m(np.array([0.0, -0.0, 3.0, -1.0], dtype=np.float32), skip_zeros=False) == 0.5
    assert m(np.zeros(5)) == 0.0 and m(np.array([])) == 0.0
    assert m(np.array([1.0, np.nan, 2.0, np.inf, 3.0])) == 3.0  # NaN sorts behind +inf
    assert adaptive_ref.SIGMA_DENOMINATOR == 0.6744897501960817


# ------------------------------------------------------------------------------------------------ the C ABI, without a GPU
def _header_text():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "pypwt_amd.h")).read()


def test_header_declares_the_new_entry_points_as_new():
    txt = _header_text()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in txt, name
    doc = txt[txt.index("NEW: adaptive denoising"):txt.index("int pdwt_band_stats_async(")]
    assert "no reference counterpart" in doc and "PDWT_DENOISE_BAYES" in doc


@pytest.mark.parametrize("variant", ["f32", "f64"])
def test_both_libraries_export_them_and_refuse_a_null_handle(variant):
    from pypwt_amd.build import build_library
    build_library(verbose=False, variant=variant)
    from pypwt_amd import _lib
    lib = _lib.load(variant)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), (variant, name)
        assert name in _lib.SIGNATURES
    table = (lib.pdwt_real * 4)()
    sigma = (C.c_double * 1)(1.0)
    assert lib.pdwt_band_stats_async(None, None) == _lib.ERR_ARG
    assert lib.pdwt_estimate_sigma_async(None, 1, None) == _lib.ERR_ARG
    assert lib.pdwt_threshold_bands(None, 0, table, 0) == _lib.ERR_ARG
    assert lib.pdwt_denoise_async(None, 0, 0, sigma, 1, 1) == _lib.ERR_ARG
    assert lib.pdwt_denoise_async(None, 0, 0, None, 0, 1) == _lib.ERR_ARG
    st = C.c_void_p()
    assert lib.pdwt_adaptive_slots(None, C.byref(st), None, None) == _lib.ERR_ARG
    assert b"null plan handle" in lib.pdwt_last_error()


def test_python_classes_have_the_new_methods():
    from pypwt_amd import BatchedWavelets, BatchedWavelets64, Wavelets, Wavelets64
    for cls in (Wavelets, Wavelets64, BatchedWavelets, BatchedWavelets64):
        for m in ("band_stats", "estimate_sigma", "threshold_bands", "denoise", "last_thresholds", "read_band_stats", "read_sigma"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    import inspect
    sig = inspect.signature(Wavelets.denoise).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("method", "BayesShrink"), ("sigma", None), ("mode", "soft"), ("skip_zeros", True)]
    assert inspect.signature(Wavelets.estimate_sigma).parameters["skip_zeros"].default is True
    assert inspect.signature(Wavelets.threshold_bands).parameters["mode"].default == "soft"
