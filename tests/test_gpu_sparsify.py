"""GPU tests of the best K-term approximation (`pytest -m gpu`): select_magnitude and keep_largest against tests/sparsify_ref.py,
in the fp32 and in the fp64 library.  Every comparison is exact: bit patterns for coefficients and thresholds, integers for
`kept`.

Plans: those of tests/test_gpu_ops.py (odd 61 x 59, SWT, 1D, batched 1D, 1D SWT), BatchedWavelets with 3 images of 61 x 59
(image borders inside a 16-byte group, a K of its own per image) and 2 of 256 x 192 db4 L2 (the finest bands span several pieces
of the sweep)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import ops_ref
import sparsify_ref as ref
from golden_util import reconstruction_tol
from oracle import oracle
from test_gpu_adaptive import DevBuf, Plan, _id, swept
from test_gpu_ops import CASES as OPS_CASES
from test_gpu_parity import flat_coeffs

pytestmark = pytest.mark.gpu

PLANS = [("w",) + c for c in OPS_CASES] + [("b", 3, 61, 59, 0, "db2", 2), ("b", 2, 256, 192, 0, "db4", 2)]
DTYPES = [np.float32, np.float64]


def read(p, view):
    """A device view of one of the plan's slots, copied to the host."""
    from pypwt_amd.wavelets import _read_device
    return _read_device(p.w._lib, p.w._h, view.ptr, view.shape, view.dtype)


def set_bands(p, bands):
    """Every band of the plan from (batch, rows, cols) arrays."""
    for num, band in enumerate(bands):
        band = np.ascontiguousarray(band)
        if p.spec[0] == "w":
            p.w.set_coeff(band.reshape(band.shape[1:]), num)
        else:
            assert p.w._lib.pdwt_set_coeff(p.w._h, band.ctypes.data_as(C.c_void_p), num, 0) == 0


def ks_of(p, k):
    """One K for a single image; for a batch a K of its own per image."""
    return int(k) if p.batch == 1 else [max(int(k) - 3 * i, 0) for i in range(p.batch)]


def assert_bands(got, want, what):
    for b, (g, r) in enumerate(zip(got, want)):
        assert ref.same_bits(g, r), (what, b)


# ---------------------------------------------------------------------------------------------------------- own coefficients
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", PLANS, ids=_id)
def test_own_coefficients(spec, dtype):
    """select_magnitude (threshold, kept) and keep_largest (every band) against the reference for K in {0, 1, N // 3, N - 1, N,
    N + 5}, with and without the approximation; the approximation is bit-identical when it is not swept; the whole-arena norms
    afterwards are the reference's, so the padding is still zero."""
    p = Plan(spec, dtype)
    bands = p.bands()
    for do_app in (0, 1):
        n = ref.count(bands, do_app)
        for k in (0, 1, n // 3, n - 1, n, n + 5):
            ks = ks_of(p, k)
            p = Plan(spec, dtype)
            t_view, k_view = p.w.select_magnitude(ks, do_threshold_appcoeffs=do_app)
            assert t_view.shape == (p.batch,) and t_view.dtype == np.dtype(dtype)
            assert k_view.shape == (p.batch,) and k_view.dtype == np.uint64
            want_t, want_kept = ref.select_magnitude(bands, ks, do_app)
            assert ref.same_bits(read(p, t_view), want_t), (do_app, k)
            assert np.array_equal(read(p, k_view), want_kept), (do_app, k)
            assert_bands(p.bands(), bands, "select_magnitude is read-only")
            p.w.keep_largest(ks, do_threshold_appcoeffs=do_app)
            thr, kept, want = ref.keep_largest(bands, ks, do_app)
            got_t, got_kept = p.w.last_sparsify()
            assert ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept), (do_app, k, got_t, thr, got_kept, kept)
            got = p.bands()
            assert_bands(got, want, (do_app, k))
            if not do_app:
                assert ref.same_bits(got[0], bands[0])
            assert np.all(kept >= np.minimum(np.asarray(ks), n))
            n1, n2 = ops_ref.norms(want)
            rel = 2.0 * sum(swept(b) for b in want) * 2.0 ** -53
            p.w.norms_device()
            s1, s2 = p.w.read_norms()
            assert abs(s1 - n1) <= rel * n1 and abs(s2 - n2) <= rel * n2, (do_app, k, s1, n1, s2, n2)


# ------------------------------------------------------------------------------------------------------- injected coefficients
def injected(p, shapes, seed):
    """Small integers with many ties, zeros and -0.0, denormals, one NaN and +-inf per image, every image its own values."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(p.dtype).type
    fi = np.finfo(dt)
    bands = []
    for num, shape in enumerate(shapes):
        v = rng.integers(-3, 4, shape).astype(dt)
        flat = v.reshape(shape[0], -1)
        flat[:, ::7] = -0.0
        flat[:, 1::11] = fi.smallest_subnormal
        flat[:, 2::13] = -np.nextafter(fi.tiny, dt(0))
        if num == len(shapes) - 1:
            for i in range(shape[0]):
                flat[i, 5 + i] = np.nan
                flat[i, 9 + i] = np.inf
                flat[i, 17 + 2 * i] = -np.inf
        bands.append(v)
    return bands


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", [PLANS[1], PLANS[2], PLANS[4], PLANS[6]], ids=_id)
def test_injected_ties_nan_inf_denormals(spec, dtype):
    p = Plan(spec, dtype)
    shapes = [b.shape for b in p.bands()]
    bands = injected(p, shapes, 13)
    for do_app in (0, 1):
        n = ref.count(bands, do_app)
        allk = np.concatenate([ref.keys(bands[b][0]).ravel() for b in ref.swept(bands, do_app)])
        at_least = lambda v: int(np.count_nonzero(allk >= ref.keys(np.array([v], dtype=dtype))[0]))
        # K = 1: the NaN is the threshold; 2: the infinities tie; inside and at both ends of the ties at 3, 2, 1, the denormals, 0
        cases = [1, 2, 3, at_least(3.0) - 1, at_least(3.0), at_least(3.0) + 1, at_least(2.0) - 1, at_least(1.0) + 1,
                 at_least(np.finfo(dtype).smallest_subnormal), at_least(np.finfo(dtype).smallest_subnormal) + 1, n - 1]
        for k in cases:
            ks = ks_of(p, k)
            set_bands(p, bands)
            p.w.keep_largest(ks, do_threshold_appcoeffs=do_app)
            thr, kept, want = ref.keep_largest(bands, ks, do_app)
            got_t, got_kept = p.w.last_sparsify()
            assert ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept), (do_app, k, got_t, thr, got_kept, kept)
            assert_bands(p.bands(), want, (do_app, k))
            if k == 1:
                assert np.isnan(got_t[0]) and got_kept[0] == 1
            if k == 2:
                assert np.isposinf(got_t[0]) and got_kept[0] == 3
            if k == at_least(3.0) - 1:
                assert got_t[0] == 3 and got_kept[0] == at_least(3.0) > k  # a tie boundary: more than K survive
            set_bands(p, bands)
            t_view, k_view = p.w.select_magnitude(ks, do_threshold_appcoeffs=do_app)
            assert ref.same_bits(read(p, t_view), thr) and np.array_equal(read(p, k_view), kept)


# ------------------------------------------------------------------------------------------- read-only, repeatable, arguments
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", [PLANS[0], PLANS[6]], ids=_id)
def test_select_is_read_only_repeatable_and_takes_fraction(spec, dtype):
    p = Plan(spec, dtype)
    bands, st = p.bands(), p.state()
    n = ref.count(bands)
    a = [read(p, v) for v in p.w.select_magnitude(n // 5)]
    b = [read(p, v) for v in p.w.select_magnitude(n // 5)]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert_bands(p.bands(), bands, "select_magnitude")
    assert p.state() == st
    # fraction = 0.1 is K = round(0.1 N), for the select and for the sweep, with and without the approximation
    for do_app in (0, 1):
        k = int(round(0.1 * ref.count(bands, do_app)))
        f = [read(p, v) for v in p.w.select_magnitude(fraction=0.1, do_threshold_appcoeffs=do_app)]
        want = ref.select_magnitude(bands, k, do_app)
        assert ref.same_bits(f[0], want[0]) and np.array_equal(f[1], want[1])
    q = Plan(spec, dtype)
    q.w.keep_largest(fraction=0.1)
    assert_bands(q.bands(), ref.keep_largest(bands, int(round(0.1 * n)))[2], "fraction")
    assert q.state() == st
    # caller-owned device slots through the C ABI; the plan's own slots keep the last call that used them
    dt, dk = DevBuf(np.zeros(p.batch, dtype=dtype)), DevBuf(np.zeros(p.batch, dtype=np.uint64))
    kk = (C.c_longlong * 1)(n // 7)
    assert p.w._lib.pdwt_select_magnitude_async(p.w._h, kk, 1, 0, C.c_void_p(dt.__cuda_array_interface__["data"][0]),
                                                C.c_void_p(dk.__cuda_array_interface__["data"][0])) == 0
    from pypwt_amd.wavelets import _read_device
    want = ref.select_magnitude(bands, n // 7)
    assert ref.same_bits(_read_device(p.w._lib, p.w._h, dt.__cuda_array_interface__["data"][0], (p.batch,), dtype), want[0])
    assert np.array_equal(_read_device(p.w._lib, p.w._h, dk.__cuda_array_interface__["data"][0], (p.batch,), np.uint64), want[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bad_arguments(dtype):
    from pypwt_amd import _lib
    p = Plan(PLANS[6], dtype)
    bands = p.bands()
    for fn in (p.w.select_magnitude, p.w.keep_largest):
        for kwargs in ({}, dict(k=3, fraction=0.5), dict(k=-1), dict(k=[1, 2]), dict(k=[1, 2, 3, 4]), dict(k=[1, -2, 3]), dict(k=2.5),
                       dict(k="many"), dict(fraction=1.5), dict(fraction=-0.1), dict(fraction=float("nan")), dict(fraction="half"),
                       dict(k=[[1, 2, 3]])):
            with pytest.raises(ValueError) as e:
                fn(**kwargs)
            assert "expected exactly one of k" in str(e.value) and "3 ints" in str(e.value), kwargs
    lib, h = p.w._lib, p.w._h
    good, neg = (C.c_longlong * 3)(1, 2, 3), (C.c_longlong * 3)(1, -2, 3)
    assert lib.pdwt_select_magnitude_async(h, None, 1, 0, None, None) == _lib.ERR_ARG
    assert lib.pdwt_select_magnitude_async(h, good, 2, 0, None, None) == _lib.ERR_ARG
    assert lib.pdwt_select_magnitude_async(h, good, 0, 0, None, None) == _lib.ERR_ARG
    assert lib.pdwt_select_magnitude_async(h, neg, 3, 0, None, None) == _lib.ERR_ARG
    assert lib.pdwt_keep_largest_async(h, None, 3, 0) == _lib.ERR_ARG
    assert lib.pdwt_keep_largest_async(h, good, 4, 0) == _lib.ERR_ARG
    assert lib.pdwt_keep_largest_async(h, neg, 3, 0) == _lib.ERR_ARG
    assert "negative" in _lib.last_error(lib)
    assert lib.pdwt_keep_largest_async(h, good, 3, 0) == 0 and lib.pdwt_keep_largest_async(h, good, 1, 1) == 0
    assert_bands(p.bands(), ref.keep_largest(ref.keep_largest(bands, [1, 2, 3])[2], 1, 1)[2], "the two calls through the C ABI")


# ------------------------------------------------------------------------------------------------------------- 2D SWT plans
SWT = ("w", (64, 96), 2, 1, "db2", 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_deferred_soft_threshold_is_settled_first(dtype):
    """soft_threshold(beta) on a 2D SWT plan is deferred into the inverse: keep_largest sees the thresholded bands, and
    inverse() then returns the oracle's inverse of the sparsified bands."""
    beta = 6.0
    p = Plan(SWT, dtype)
    raw = p.bands()
    thr = [adaptive_ref.images(b, 1) for b in ops_ref.threshold([b[0] for b in raw], p.levels, 2, "soft", beta)]
    k = ref.count(thr) // 20
    p.w.soft_threshold(beta)
    t_view, k_view = p.w.select_magnitude(k)
    want_t, want_kept, want = ref.keep_largest(thr, k)
    assert ref.same_bits(read(p, t_view), want_t) and np.array_equal(read(p, k_view), want_kept)
    p = Plan(SWT, dtype)
    st = p.state()
    p.w.soft_threshold(beta)
    p.w.keep_largest(k)
    assert p.state() == st
    got_t, got_kept = p.w.last_sparsify()
    assert ref.same_bits(got_t, want_t) and np.array_equal(got_kept, want_kept)
    assert_bands(p.bands(), want, "soft_threshold, keep_largest")
    if dtype != np.float32:
        return  # the oracle's inverse is fp32
    p = Plan(SWT, dtype)
    p.w.soft_threshold(beta)
    p.w.keep_largest(k)
    p.w.inverse()
    rec = oracle.inverse([b[0] for b in want], p.x.shape, p.wname, p.levels, do_swt=1)
    assert np.abs(p.w.image - rec).max() <= reconstruction_tol(p.x, p.wname, p.levels, do_swt=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_after_inverse_keep_largest_warns_and_changes_nothing(dtype, capsys):
    from pypwt_amd import _lib
    p = Plan(SWT, dtype)
    p.w.soft_threshold(6.0)
    p.w.inverse()
    img, st = p.image(), p.state()
    capsys.readouterr()
    p.w.keep_largest(10)
    out = capsys.readouterr().out
    assert out.count("Warning") == 1 and "modified by inverse()" in out
    kk = (C.c_longlong * 1)(10)
    assert p.w._lib.pdwt_keep_largest_async(p.w._h, kk, 1, 0) == _lib.ERR_STATE
    assert np.array_equal(p.image(), img) and p.state() == st
    # the read-only select runs in every state, as band_stats does
    t, kept = [read(p, v) for v in p.w.select_magnitude(10)]
    assert kept[0] >= 10 and t[0] >= 0 and p.state() == st
    assert np.array_equal(p.image(), img)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_clone_carries_the_sparsified_bands(dtype):
    p = Plan(SWT, dtype)
    raw = p.bands()
    thr = [adaptive_ref.images(b, 1) for b in ops_ref.threshold([b[0] for b in raw], p.levels, 2, "soft", 4.0)]
    k = ref.count(thr) // 9
    p.w.soft_threshold(4.0)
    p.w.keep_largest(k)
    want = ref.keep_largest(thr, k)[2]
    lib = p.w._lib
    twin = C.c_void_p()
    assert lib.pdwt_clone(p.w._h, C.byref(twin)) == 0
    try:
        for num, r in enumerate(want):
            got = np.zeros(r.shape, dtype=dtype)
            assert lib.pdwt_get_coeff(twin, got.ctypes.data_as(C.c_void_p), num) == r.size
            assert ref.same_bits(got, r), num
    finally:
        lib.pdwt_destroy(twin)
    assert_bands(p.bands(), want, "the source after clone")


# ---------------------------------------------------------------------------------------------------------------- bindings
def test_ctypes_and_cython_classes_give_the_same_bits():
    from pypwt_amd import build
    so = build.build_cython(verbose=False)
    if not so:
        pytest.skip("cython is not installed")
    from pypwt_amd._cy import Wavelets as Cy
    from pypwt_amd.wavelets import Wavelets as Ct
    x = oracle.hash_input((192, 160), 77, 100.0) - 50.0
    for kwargs in (dict(k=1000), dict(fraction=0.05, do_threshold_appcoeffs=1), dict(k=0), dict(k=10 ** 9)):
        a, b = Cy(x, "db3", 3), Ct(x, "db3", 3)
        a.forward(); b.forward()
        a.select_magnitude(**kwargs); b.select_magnitude(**kwargs)
        (ta, ka), (tb, kb) = a.last_sparsify(), b.last_sparsify()
        assert ta.tobytes() == tb.tobytes() and ka.tobytes() == kb.tobytes() and ka.dtype == np.uint64 and ta.dtype == np.float32
        a.keep_largest(**kwargs); b.keep_largest(**kwargs)
        (ta, ka), (tb, kb) = a.last_sparsify(), b.last_sparsify()
        assert ta.tobytes() == tb.tobytes() and ka.tobytes() == kb.tobytes()
        for g, h in zip(flat_coeffs(a), flat_coeffs(b)):
            assert ref.same_bits(g, h)
        a.inverse(); b.inverse()
        assert np.array_equal(a.image, b.image)
        a.keep_largest(k=5)  # after inverse(): a warning, nothing else
        assert np.array_equal(a.image, b.image)
    for kwargs in ({}, dict(k=1, fraction=0.5), dict(k=-1), dict(fraction=2.0), dict(k=[1, 2])):
        with pytest.raises(ValueError):
            a.select_magnitude(**kwargs)


# ------------------------------------------------------------------------------------------- the shared select workspace
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", [PLANS[1], PLANS[6]], ids=_id)
def test_estimate_sigma_and_keep_largest_leave_the_select_workspace_clean(spec, dtype):
    p = Plan(spec, dtype)
    bands = p.bands()
    noise = adaptive_ref.noise_band(p.ndim)
    k = ks_of(p, ref.count(bands) // 4)
    # estimate_sigma, keep_largest, estimate_sigma: each against its reference
    assert np.array_equal(p.w.read_sigma(p.w.estimate_sigma()), adaptive_ref.estimate_sigma(bands[noise]))
    p.w.keep_largest(k)
    thr, kept, want = ref.keep_largest(bands, k)
    got_t, got_kept = p.w.last_sparsify()
    assert ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept)
    assert_bands(p.bands(), want, "keep_largest after estimate_sigma")
    for skip in (True, False):
        assert np.array_equal(p.w.read_sigma(p.w.estimate_sigma(skip_zeros=skip)), adaptive_ref.estimate_sigma(want[noise], skip))
    # ... and a select right behind it
    t, c = [read(p, v) for v in p.w.select_magnitude(k)]
    thr2, kept2 = ref.select_magnitude(want, k)
    assert ref.same_bits(t, thr2) and np.array_equal(c, kept2)
