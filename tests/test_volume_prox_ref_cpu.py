"""tests/volume_prox_ref.py pinned to things that are not it, and the six proximal entry points of a volume checked without a GPU:
declared with a citation, exported by both libraries, bound, documented, and PDWT_ERR_ARG for a null handle.

  * regrouped as three-band groups, `group_soft` is tests/ops_ref.py's group_soft of a 2D plan, bit for bit;
  * a group of norm <= beta becomes exactly zero, one above it keeps its direction and has the norm ||g|| - beta;
  * Moreau: soft(c, beta) + linf(c, beta) == c within one ulp of |c|;
  * `group_norm` of a volume with one non-zero member per group is the l1 norm.
"""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import ops_ref
import volume_prox_ref as prox
import volume_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pdwt_volume_group_soft_threshold", "pdwt_volume_proj_linf", "pdwt_volume_shrink", "pdwt_volume_add_wavelet",
               "pdwt_volume_group_norm", "pdwt_volume_group_norm_async"]
DTYPES = [np.float32, np.float64]


def bands_of(shape, levels, dtype, seed, scale=10.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(s) * scale).astype(dtype) for s in volume_ref.band_shapes(shape, levels)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_groups_of_three_are_the_2d_plans_group_soft(dtype):
    rng = np.random.default_rng(3)
    levels = 3
    bands = [(rng.standard_normal((6, 5)) * 4.0).astype(dtype) for _ in range(1 + 3 * levels)]
    for do_app in (0, 1):
        for normalize in (0, 1):
            got = prox.group_soft(bands, levels, 5.5, do_app, normalize, per=3)
            want, _ = ops_ref.group_soft(bands, levels, 2, 5.5, do_app, normalize)
            assert all(ops_ref.same_bits(g, w) for g, w in zip(got, want)), (do_app, normalize)
    assert prox.groups(2, 1) == [[1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 0]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_groups_vanish_and_large_ones_keep_their_direction(dtype):
    shape, levels, beta = (9, 10, 13), 2, 26.0
    bands = bands_of(shape, levels, dtype, 5)
    eps = float(np.finfo(dtype).eps)
    for do_app in (0, 1):
        out = prox.group_soft(bands, levels, beta, do_app)
        frac = prox.zeroed_fraction(bands, levels, beta, do_app)
        assert 0.1 < frac < 0.9
        for idx in prox.groups(levels, do_app):
            g = np.stack([bands[i].astype(np.longdouble) for i in idx])
            o = np.stack([out[i].astype(np.longdouble) for i in idx])
            nrm, onrm = np.sqrt((g * g).sum(0)), np.sqrt((o * o).sum(0))
            small = nrm <= beta
            assert small.any() and (~small).any()
            assert np.all(o[:, small] == 0)
            # ||out|| = ||g|| - beta and out is parallel to g, up to the rounding of the members to the band's type
            assert np.all(np.abs(onrm[~small] - (nrm[~small] - beta)) <= 4 * eps * nrm[~small])
            cos = (g * o).sum(0)[~small] / (nrm[~small] * np.maximum(onrm[~small], np.finfo(np.longdouble).tiny))
            big = onrm[~small] > 1e-3 * nrm[~small]  # (a direction needs a length)
            assert np.all(np.abs(cos[big] - 1) <= 1e3 * eps)
        if not do_app:
            assert np.array_equal(out[0], bands[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_moreau_soft_plus_linf_is_the_identity_within_one_ulp(dtype):
    bands = bands_of((6, 6, 10), 1, dtype, 7)
    bands.append(ops_ref.edge_vector(3.25, dtype, finite_only=True))
    for beta in (3.25, 0.0, 40.0):
        for b in bands:
            s, p = ops_ref.soft(b, beta), ops_ref.linf(b, beta)
            with np.errstate(over="ignore"):
                ulp = np.spacing(np.abs(b))  # (inf at the largest finite value)
            assert np.all(np.abs((s + p).astype(np.longdouble) - b.astype(np.longdouble)) <= ulp), beta
    out = prox.linf(bands[:8], 3.25, 0)
    assert np.array_equal(out[0], bands[0]) and float(np.abs(out[1]).max()) == 3.25
    out = prox.shrink(bands[:8], 0.25, 0)
    assert np.array_equal(out[0], bands[0]) and np.array_equal(out[3], bands[3] * dtype(dtype(1) / dtype(1.25)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_with_one_member_per_group_is_the_l1_norm(dtype):
    shape, levels = (7, 5, 6), 2
    bands = bands_of(shape, levels, dtype, 9)
    rng = np.random.default_rng(11)
    for l in range(1, levels + 1):
        idx = prox.groups(levels, 1)[l - 1]
        keep = rng.integers(0, len(idx), bands[idx[0]].shape)
        for k, i in enumerate(idx):
            bands[i][keep != k] = 0
    n1, _ = ops_ref.norms(bands)
    got = prox.group_norm(bands, levels, 1)
    assert abs(got - np.longdouble(n1)) <= 4 * float(np.finfo(np.float64).eps) * n1
    # without A_L the groups of the last level lose the positions A_L held
    lost = float(np.abs(bands[0].astype(np.float64)).sum())
    assert abs(prox.group_norm(bands, levels, 0) - np.longdouble(n1 - lost)) <= 8 * float(np.finfo(np.float64).eps) * n1


# ------------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_header_declares_and_cites_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "pypwt_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert ("int %s(" % name) in txt, name
        doc = txt[txt.index("The proximal operators and the linear combination"):]
        at = doc.index(name)
        near = doc[at:at + 400]
        assert "wt.cu:" in near or "common.cu:" in near or "no reference counterpart" in near, name
    scope = txt[txt.index("Out of scope: 3D SWT"):txt.index("typedef struct pdwt_volume* pdwt_volume_handle;")]
    assert "shrink / group" not in scope
    bench = open(os.path.join(ROOT, "include", "pypwt_amd_bench.h")).read()
    assert not any(name in bench for name in NEW_SYMBOLS)


def test_integration_document_names_the_calls():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in doc, name
    for m in ("group_soft_threshold", "proj_linf", "shrink", "add_wavelet", "group_norm", "group_norm_device"):
        assert m in doc, m
    from pypwt_amd.build import CY_DIR, cython_extern_block
    assert open(os.path.join(CY_DIR, "pdwt_decl.pxi")).read() == cython_extern_block()


@pytest.mark.parametrize("variant", ["f32", "f64"])
def test_both_libraries_export_them_and_refuse_a_null_handle(variant):
    from pypwt_amd.build import build_library
    build_library(verbose=False, variant=variant)
    from pypwt_amd import _lib
    lib = _lib.load(variant)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), (variant, name)
        assert name in _lib.SIGNATURES
    out = C.c_double(7.0)
    slot = C.c_void_p()
    assert lib.pdwt_volume_group_soft_threshold(None, 1.0, 0, 0) == _lib.ERR_ARG
    assert lib.pdwt_volume_proj_linf(None, 1.0, 1) == _lib.ERR_ARG
    assert lib.pdwt_volume_shrink(None, 1.0, 1) == _lib.ERR_ARG
    assert lib.pdwt_volume_add_wavelet(None, None, 1.0) == _lib.ERR_ARG
    assert lib.pdwt_volume_group_norm(None, 0, C.byref(out)) == _lib.ERR_ARG
    assert lib.pdwt_volume_group_norm_async(None, 0, None, C.byref(slot)) == _lib.ERR_ARG
    assert b"null" in lib.pdwt_last_error()
    assert out.value == 7.0 and not slot.value


def test_python_classes_have_the_methods_with_wavelets_signatures():
    from pypwt_amd import Wavelets, Wavelets3D, Wavelets3D64
    for m in ("group_soft_threshold", "proj_linf", "shrink", "add_wavelet"):
        got = inspect.signature(getattr(Wavelets3D, m)).parameters
        want = inspect.signature(getattr(Wavelets, m)).parameters
        assert [(k, v.default) for k, v in got.items()] == [(k, v.default) for k, v in want.items()], m
    sig = {m: [(k, v.default) for k, v in inspect.signature(getattr(Wavelets3D, m)).parameters.items()][1:]
           for m in ("group_norm", "group_norm_device", "proj_linf", "shrink", "group_soft_threshold")}
    assert sig["group_norm"] == [("do_threshold_appcoeffs", 0)]
    assert sig["group_norm_device"][0] == ("out", None)
    assert sig["proj_linf"] == sig["shrink"] == [("beta", inspect.Parameter.empty), ("do_threshold_appcoeffs", 1)]
    assert sig["group_soft_threshold"] == [("beta", inspect.Parameter.empty), ("do_threshold_appcoeffs", 0), ("normalize", 0)]
    for m in ("group_soft_threshold", "proj_linf", "shrink", "add_wavelet", "group_norm", "group_norm_device"):
        assert getattr(Wavelets3D64, m) is getattr(Wavelets3D, m)
    doc = Wavelets3D.__doc__
    refused = doc[doc.index("The operators that choose a threshold"):doc.index("NotImplementedError")]
    assert "norms_device" in refused and not any(m in refused for m in ("group_", "proj_linf", "shrink", "add_wavelet"))
