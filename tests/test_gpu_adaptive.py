"""GPU tests of the adaptive denoising operators (`pytest -m gpu`): band_stats, estimate_sigma, threshold_bands, denoise against
tests/adaptive_ref.py on the plan's OWN coefficients read back after forward(), in the fp32 and in the fp64 library.

Plans: those of tests/test_gpu_ops.py (odd 61 x 59, SWT, 1D, batched 1D), BatchedWavelets with 3 images of 61 x 59 (image
borders inside a 16-byte group) and 16 of 512^2, and one 4096^2 db4 L4 plan."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
from adaptive_check import _id, check_table, swept
import ops_ref
from golden_util import reconstruction_tol
from oracle import oracle
from test_gpu_ops import CASES as OPS_CASES, _hip
from test_gpu_parity import flat_coeffs

pytestmark = pytest.mark.gpu

# ("w", shape, ndim, swt, wavelet, levels): Wavelets;  ("b", batch, Nr, Nc, swt, wavelet, levels): BatchedWavelets
PLANS = [("w",) + c for c in OPS_CASES] + [("b", 3, 61, 59, 0, "db2", 2), ("b", 16, 512, 512, 0, "db4", 3),
                                           ("w", (4096, 4096), 2, 0, "db4", 4)]
SMALL = PLANS[:7]
DTYPES = [np.float32, np.float64]


class Plan(object):
    """A plan after forward(), its coefficients as (batch, rows, cols) bands, and what the tests need to know about it."""

    def __init__(self, spec, dtype, seed=1, x=None):
        import pypwt_amd
        self.spec, self.dtype = spec, dtype
        f64 = dtype == np.float64
        if spec[0] == "w":
            _, shape, nd, swt, wname, lv = spec
            self.x = (oracle.hash_input(shape, seed, 100.0) - 50.0).astype(dtype) if x is None else x.astype(dtype)
            cls = pypwt_amd.Wavelets64 if f64 else pypwt_amd.Wavelets
            self.w = cls(self.x[0] if shape[0] == 1 else self.x, wname, lv, do_swt=swt, ndim=nd)
            self.batch, self.ndim, self.swt, self.wname, self.levels = 1, nd, swt, wname, self.w.levels
            self.nsamples = shape[0] * shape[1]
        else:
            _, batch, Nr, Nc, swt, wname, lv = spec
            self.x = (oracle.hash_input((batch * Nr, Nc), seed, 100.0) - 50.0).astype(dtype).reshape(batch, Nr, Nc)
            cls = pypwt_amd.BatchedWavelets64 if f64 else pypwt_amd.BatchedWavelets
            self.w = cls(batch, Nr, Nc, wname, lv, do_swt=swt, img=self.x)
            self.batch, self.ndim, self.swt, self.wname, self.levels = batch, 2, swt, wname, self.w.levels
            self.nsamples = Nr * Nc
        self.w.forward()
        self.nbands = (3 if self.ndim == 2 else 1) * self.levels + 1

    def bands(self):
        if self.spec[0] == "w":
            return [adaptive_ref.images(b, 1).copy() for b in flat_coeffs(self.w)]
        return [self.w.coeff(k) for k in range(self.nbands)]

    def state(self):
        from pypwt_amd._lib import PdwtInfo
        info, st = PdwtInfo(), C.c_int()
        self.w._lib.pdwt_get_info(self.w._h, C.byref(info), None, None, C.byref(st), None)
        return st.value

    def image(self):
        return self.w.image.copy()


_REF = {}


def ref_of(plan):
    """Reference sums and noise levels of a plan's coefficients (cached: the coefficients of a spec are the same every time)."""
    key = (plan.spec, np.dtype(plan.dtype).name)
    if key not in _REF:
        bands = plan.bands()
        nb = bands[adaptive_ref.noise_band(plan.ndim)]
        _REF[key] = dict(stats=adaptive_ref.band_stats(bands), sigma=adaptive_ref.estimate_sigma(nb, True),
                         sigma_all=adaptive_ref.estimate_sigma(nb, False))
    return _REF[key]


class DevBuf(object):
    """A hipMalloc'ed buffer with __cuda_array_interface__ (what a torch tensor or a cupy array exposes)."""

    def __init__(self, host):
        self._hip = _hip()
        self._p = C.c_void_p()
        host = np.ascontiguousarray(host)
        assert self._hip.hipMalloc(C.byref(self._p), host.nbytes) == 0
        assert self._hip.hipMemcpy(self._p, host.ctypes.data, host.nbytes, 1) == 0
        self.__cuda_array_interface__ = {"shape": host.shape, "typestr": host.dtype.str, "data": (self._p.value, False),
                                         "version": 3, "strides": None}

    def __del__(self):
        self._hip.hipFree(self._p)


# ------------------------------------------------------------------------------------------------------------ band_stats
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", PLANS, ids=_id)
def test_band_stats(spec, dtype):
    """Every entry within n 2^-53 times 2 (n the swept length of that band) of the exact sum, relative to the sum of the
    absolute terms (the terms are non-negative: the sum itself); their total equals norms_device within the bound
    test_gpu_ops.py derives for it; two calls give identical bits."""
    p = Plan(spec, dtype)
    bands = p.bands()
    ref = ref_of(p)["stats"]
    view = p.w.band_stats()
    assert view.shape == (p.nbands, p.batch, 2) and view.dtype == np.float64
    got = p.w.read_band_stats(view)
    again = p.w.read_band_stats(p.w.band_stats())
    assert got.tobytes() == again.tobytes()
    worst = 0.0
    for b in range(p.nbands):
        bound = 2.0 * swept(bands[b]) * 2.0 ** -53
        for i in range(p.batch):
            for k in range(2):
                err = abs(got[b, i, k] - ref[b, i, k])
                worst = max(worst, err / max(ref[b, i, k], 1e-300) / bound)
                assert err <= bound * ref[b, i, k], (b, i, k, got[b, i, k], ref[b, i, k])
    print("band_stats %s %s: worst error %.3f of the bound" % (_id(spec), np.dtype(dtype).name, worst))
    p.w.norms_device()
    n1, n2 = p.w.read_norms()
    rel = 2.0 * sum(swept(b) for b in bands) * 2.0 ** -53
    assert abs(got[:, :, 0].sum() - n1) <= rel * n1 and abs(got[:, :, 1].sum() - n2) <= rel * n2
    # a caller-owned slot
    out = DevBuf(np.zeros((p.nbands, p.batch, 2)))
    assert p.w.band_stats(out=out) is out
    assert p.w.read_band_stats(out).tobytes() == got.tobytes()


# -------------------------------------------------------------------------------------------------------- estimate_sigma
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", PLANS, ids=_id)
def test_estimate_sigma_is_exact(spec, dtype):
    p = Plan(spec, dtype)
    ref = ref_of(p)
    v = p.w.estimate_sigma()
    assert v.shape == (p.batch,) and v.dtype == np.float64
    got = p.w.read_sigma(v)
    assert np.array_equal(got, ref["sigma"]), (got, ref["sigma"])
    got = p.w.read_sigma(p.w.estimate_sigma(skip_zeros=False))
    assert np.array_equal(got, ref["sigma_all"]), (got, ref["sigma_all"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", [PLANS[1], PLANS[3], PLANS[6]], ids=_id)
def test_estimate_sigma_on_edge_values(spec, dtype):
    """The noise band set from ops_ref.edge_vector (signed zeros, denormals, +-max, +-inf, NaN, ties) and from vectors with many
    zeros and ties, every image with its own values."""
    p = Plan(spec, dtype)
    num = adaptive_ref.noise_band(p.ndim)
    shape = p.bands()[num].shape
    n = int(np.prod(shape[1:]))
    rng = np.random.default_rng(7)
    for kind in range(3):
        imgs = []
        for i in range(p.batch):
            if kind == 0:
                v = ops_ref.tile(ops_ref.edge_vector(2.5 + i, dtype, seed=5 + i), n)
            elif kind == 1:
                v = rng.integers(-3, 4, n).astype(dtype)          # ties, and a third of the values are zeros
                v[::5] = -0.0
            else:
                v = np.zeros(n, dtype=dtype)                        # nothing left with skip_zeros ...
                v[: i + 1] = 4.0 if i % 2 else 0.0                  # ... or an odd / even handful
            imgs.append(rng.permutation(v))
        band = np.stack(imgs).reshape(shape)
        if spec[0] == "w":
            p.w.set_coeff(band.reshape(shape[1:]), num)
        else:
            p.w._lib.pdwt_set_coeff(p.w._h, band.ctypes.data_as(C.c_void_p), num, 0)
        for skip in (True, False):
            got = p.w.read_sigma(p.w.estimate_sigma(skip_zeros=skip))
            want = adaptive_ref.estimate_sigma(band, skip)
            assert np.array_equal(got, want, equal_nan=True), (kind, skip, got, want)


# ------------------------------------------------------------------------------------------------------- threshold_bands
def _table(p, seed=3):
    rng = np.random.default_rng(seed)
    T = (rng.uniform(0.5, 30.0, (p.nbands, p.batch))).astype(p.dtype)
    T[0, :] = np.nan
    T[p.nbands - 1, p.batch - 1] = np.nan
    T[1, 0] = 0.0
    return T


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("op", ["soft", "hard"])
@pytest.mark.parametrize("spec", SMALL + [PLANS[7]], ids=_id)
def test_threshold_bands_bit_identical(spec, op, dtype):
    """Table from host and from device memory; NaN entries leave their (band, image) untouched bit for bit."""
    for where in ("host", "device"):
        p = Plan(spec, dtype)
        bands = p.bands()
        T = _table(p)
        want = adaptive_ref.threshold_bands(bands, T, op)
        p.w.threshold_bands(T if where == "host" else DevBuf(T), op)
        for b, (g, r) in enumerate(zip(p.bands(), want)):
            assert ops_ref.same_bits(g, r), (where, b)
        assert ops_ref.same_bits(p.bands()[0], bands[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", [PLANS[1], PLANS[2], PLANS[6]], ids=_id)
def test_threshold_bands_row_table_negative_entries_and_padding(spec, dtype):
    """A (nbands,) table is one row for all images; a negative entry is accepted (soft(x, b) grows |x| by |b|) and the zero
    padding behind the bands stays zero: the whole-arena norms afterwards are the reference's."""
    p = Plan(spec, dtype)
    bands = p.bands()
    row = np.full(p.nbands, -1.5, dtype=dtype)
    row[0] = np.nan
    row[2] = 3.0
    p.w.threshold_bands(row, "soft")
    want = adaptive_ref.threshold_bands(bands, row, "soft")
    for g, r in zip(p.bands(), want):
        assert ops_ref.same_bits(g, r)
    n1, n2 = ops_ref.norms(want)
    rel = 2.0 * sum(swept(b) for b in want) * 2.0 ** -53
    p.w.norms_device()
    got = p.w.read_norms()
    assert abs(got[0] - n1) <= rel * n1 and abs(got[1] - n2) <= rel * n2, (got, n1, n2)
    with pytest.raises(ValueError):
        p.w.threshold_bands(np.zeros(p.nbands + 1, dtype=dtype))


# --------------------------------------------------------------------------------------------------------------- denoise
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("method,op", [("BayesShrink", "soft"), ("VisuShrink", "hard")])
@pytest.mark.parametrize("spec", PLANS, ids=_id)
def test_denoise_in_two_steps(spec, method, op, dtype):
    """First the table of last_thresholds() against the reference's, then the coefficients: bit-identical to the reference
    sweep applied with the DEVICE's table."""
    p = Plan(spec, dtype)
    bands = p.bands()
    ref = ref_of(p)
    p.w.denoise(method=method, mode=op)
    sigma, T = p.w.last_thresholds()
    assert np.array_equal(sigma, ref["sigma"])
    check_table(p, bands, sigma, T, method, ref["stats"])
    want = adaptive_ref.threshold_bands(bands, T, op)
    for b, (g, r) in enumerate(zip(p.bands(), want)):
        assert ops_ref.same_bits(g, r), b


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("spec", [PLANS[0], PLANS[6]], ids=_id)
def test_denoise_with_a_given_sigma(spec, dtype):
    """sigma from the host: one value for all images, or one per image; skip_zeros=False reaches the estimate."""
    for given in (7.25, [3.0 + i for i in range(Plan(spec, dtype).batch)]):
        p = Plan(spec, dtype)
        bands = p.bands()
        p.w.denoise(sigma=given)
        sigma, T = p.w.last_thresholds()
        assert np.array_equal(sigma, np.broadcast_to(np.asarray(given, dtype=np.float64), (p.batch,)))
        check_table(p, bands, sigma, T, "BayesShrink", ref_of(p)["stats"])
        for g, r in zip(p.bands(), adaptive_ref.threshold_bands(bands, T, "soft")):
            assert ops_ref.same_bits(g, r)
    p = Plan(spec, dtype)
    p.w.denoise(method="VisuShrink", skip_zeros=False)
    assert np.array_equal(p.w.last_thresholds()[0], ref_of(p)["sigma_all"])
    with pytest.raises(ValueError):
        p.w.denoise(sigma=[1.0] * (p.batch + 1))
    with pytest.raises(ValueError):
        p.w.denoise(method="SureShrink")


# ----------------------------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_after_inverse_the_sweeps_warn_and_change_nothing(dtype, capsys):
    p = Plan(PLANS[0], dtype)
    p.w.denoise()
    before_T = p.w.last_thresholds()
    p.w.inverse()
    img, st = p.image(), p.state()
    capsys.readouterr()
    p.w.threshold_bands(np.full(p.nbands, 5.0, dtype=dtype))
    p.w.denoise(method="VisuShrink")
    out = capsys.readouterr().out
    assert out.count("Warning") == 2 and "modified by inverse()" in out
    assert np.array_equal(p.image(), img) and p.state() == st
    after_T = p.w.last_thresholds()
    assert np.array_equal(before_T[0], after_T[0]) and np.array_equal(before_T[1], after_T[1], equal_nan=True)
    # the read-only operators behave as norms_device does there: they run, and agree with it
    stats = p.w.read_band_stats(p.w.band_stats())
    p.w.norms_device()
    n1, n2 = p.w.read_norms()
    assert abs(stats[:, :, 0].sum() - n1) <= 1e-12 * n1 and abs(stats[:, :, 1].sum() - n2) <= 1e-12 * n2
    assert np.isfinite(p.w.read_sigma(p.w.estimate_sigma())).all()
    assert p.state() == st


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_deferred_soft_threshold_is_seen_and_composes(dtype):
    """On a 2D SWT plan soft_threshold is deferred into the inverse: band_stats / estimate_sigma see the thresholded
    coefficients, and soft_threshold, denoise, inverse equals the host model."""
    spec = ("w", (64, 96), 2, 1, "db2", 2)
    beta = 6.0
    p = Plan(spec, dtype)
    raw = p.bands()
    thr = [adaptive_ref.images(b, 1) for b in ops_ref.threshold([b[0] for b in raw], p.levels, 2, "soft", beta)]
    for which in ("stats", "sigma"):
        p = Plan(spec, dtype)
        p.w.soft_threshold(beta)
        if which == "stats":
            got = p.w.read_band_stats(p.w.band_stats())
            ref = adaptive_ref.band_stats(thr)
            for b in range(p.nbands):
                bound = 2.0 * swept(thr[b]) * 2.0 ** -53
                assert np.all(np.abs(got[b] - ref[b]) <= bound * ref[b]), b
        else:
            assert np.array_equal(p.w.read_sigma(p.w.estimate_sigma()), adaptive_ref.estimate_sigma(thr[3]))
        st = p.state()
        assert st == Plan(spec, dtype).state()  # none of them changes the plan's state
    if dtype != np.float32:
        return  # the oracle's inverse is fp32
    p = Plan(spec, dtype)
    p.w.soft_threshold(beta)
    p.w.denoise()
    sigma, T = p.w.last_thresholds()
    p.w.inverse()
    _, T_ref, den = adaptive_ref.denoise(thr, 2, p.nsamples)
    assert np.array_equal(sigma, adaptive_ref.estimate_sigma(thr[3]))
    want = oracle.inverse([b[0] for b in den], p.x.shape, p.wname, p.levels, do_swt=1)
    assert np.abs(p.w.image - want).max() <= reconstruction_tol(p.x, p.wname, p.levels, do_swt=1)


# -------------------------------------------------------------------------------------------------------------- bindings
def test_ctypes_and_cython_classes_give_the_same_bits():
    from pypwt_amd import build
    so = build.build_cython(verbose=False)
    if not so:
        pytest.skip("cython is not installed")
    from pypwt_amd._cy import Wavelets as Cy
    from pypwt_amd.wavelets import Wavelets as Ct
    x = oracle.hash_input((192, 160), 77, 100.0) - 50.0
    for method, mode in (("BayesShrink", "soft"), ("VisuShrink", "hard")):
        a, b = Cy(x, "db3", 3), Ct(x, "db3", 3)
        a.forward(); b.forward()
        a.band_stats(); sb = b.band_stats()
        assert a.read_band_stats().tobytes() == b.read_band_stats(sb).tobytes()
        a.estimate_sigma(); b.estimate_sigma()
        assert a.read_sigma().tobytes() == b.read_sigma().tobytes()
        a.denoise(method=method, mode=mode); b.denoise(method=method, mode=mode)
        (sa, ta), (sb, tb) = a.last_thresholds(), b.last_thresholds()
        assert sa.tobytes() == sb.tobytes() and ta.tobytes() == tb.tobytes()
        for g, h in zip(flat_coeffs(a), flat_coeffs(b)):
            assert ops_ref.same_bits(g, h)
        row = np.array([np.nan] + [2.0] * 9, dtype=np.float32)
        a.threshold_bands(row, "hard"); b.threshold_bands(row, "hard")
        a.inverse(); b.inverse()
        assert np.array_equal(a.image, b.image)
        a.denoise()  # after inverse(): a warning, nothing else


# ------------------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_denoising_of_a_noisy_pattern():
    """512^2 smooth pattern + sigma = 10 Gaussian noise, db4 L3: forward, denoise, inverse.  The estimated sigma is within the
    sampling error of a median of 65 536 Gaussian magnitudes -- 10 * 1.17 * 4 / sqrt(65536) = 0.18 at four standard errors -- plus
    what the pattern itself puts into D1: shifting every sample by at most max |D1(pattern)| moves the median of the
    magnitudes by at most that much.  The result is closer to the clean image than the noisy one (a sanity check)."""
    from pypwt_amd import Wavelets
    r, c = np.meshgrid(np.arange(512), np.arange(512), indexing="ij")
    # whole periods along both axes: the transform is periodic, so the pattern has no edge and is smooth everywhere
    clean = (100.0 * np.sin(2 * np.pi * 5 * c / 512.0) * np.cos(2 * np.pi * 8 * r / 512.0) + 128.0).astype(np.float32)
    noisy = (clean + 10.0 * np.random.default_rng(42).standard_normal(clean.shape)).astype(np.float32)
    w0 = Wavelets(clean, "db4", 3)
    w0.forward()
    own = float(np.abs(w0.coeffs[1][2]).max())
    w = Wavelets(noisy, "db4", 3)
    w.forward()
    w.denoise()
    sigma, T = w.last_thresholds()
    w.inverse()
    allowed = 10.0 * 1.17 * 4 / np.sqrt(65536.0) + own / adaptive_ref.SIGMA_DENOMINATOR
    print("estimated sigma %.4f (allowed +-%.4f; the pattern's own D1 reaches %.4f)" % (sigma[0], allowed, own))
    assert abs(sigma[0] - 10.0) <= allowed
    mse_in = float(np.mean((noisy.astype(np.float64) - clean) ** 2))
    mse_out = float(np.mean((w.image.astype(np.float64) - clean) ** 2))
    print("mse noisy %.3f -> denoised %.3f" % (mse_in, mse_out))
    assert mse_out < mse_in
