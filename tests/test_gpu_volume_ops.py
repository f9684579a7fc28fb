"""GPU tests of the adaptive and K-term operators of `Wavelets3D` (`pytest -m gpu`): band_stats, norms_device, estimate_sigma,
threshold_bands, denoise, select_magnitude, keep_largest against tests/volume_ops_ref.py on the volume's OWN sub-bands read back
after forward(), in the fp32 and (second and fourth case) the fp64 library.

A volume is one image; the depth-low half of band A of every level below the last is an intermediate that no operator may read
or write: the tests read it straight out of the level's arena (it sits in front of the 'daa' sub-band) before and after.

Bounds: band_stats 2 n 2^-53 relative (n elements, fp64 accumulation in another order); the threshold table by
tests/test_gpu_adaptive.py's check_table rule (final rounding + A n 2^-52, A = m / |m - var|; a sub-band within the sum bound of
the max(., eps) edge is left out, ONE per case at most); everything else is exact or bit for bit.
"""
import numpy as np
import pytest

import ops_ref
import sparsify_ref
import volume_ops_ref as ref
import volume_ref
from test_gpu_adaptive import DevBuf

pytestmark = pytest.mark.gpu

# (shape, wavelet, levels)
CASES = [((16, 16, 16), "haar", 2),
         ((9, 10, 13), "db2", 1),      # sub-band borders inside 16-byte groups
         ((5, 64, 64), "haar", 2),     # odd depth twice: 5 -> 3 -> 2
         ((64, 48, 40), "db2", 3),     # two levels of intermediates
         ((6, 260, 252), "db2", 1),    # slices of 16 380 values: several pieces each
         ((24, 20, 28), "db4", 1)]
PARAMS = [(c, np.float32) for c in CASES] + [(CASES[1], np.float64), (CASES[3], np.float64)]
IDS = ["%dx%dx%d-%s-L%d-%s" % (c[0] + (c[1], c[2], np.dtype(d).name)) for c, d in PARAMS]
SIGMA = 20.0


def clean_of(shape):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) / n for n in shape], indexing="ij")
    return 128.0 + 80.0 * np.sin(2 * np.pi * z) * np.cos(2 * np.pi * y) + 40.0 * np.cos(4 * np.pi * x) * np.sin(2 * np.pi * y)


def noisy_of(case):
    shape = case[0]
    rng = np.random.default_rng(17 * sum(shape) + case[2])
    return clean_of(shape) + SIGMA * rng.standard_normal(shape)


_REF = {}


class Vol(object):
    """A volume after forward(), and the reference quantities of its own sub-bands (computed once per case and type)."""

    def __init__(self, case, dtype):
        import pypwt_amd
        self.case, self.dtype = case, dtype
        self.shape, self.wname, levels = case
        cls = pypwt_amd.Wavelets3D64 if dtype == np.float64 else pypwt_amd.Wavelets3D
        self.W = cls(noisy_of(case).astype(dtype), self.wname, levels)
        assert self.W.levels == levels
        self.W.forward()
        self.nbands = self.W.nbands
        key = (case, np.dtype(dtype).name)
        if key not in _REF:
            bands = self.bands()
            r = dict(bands=bands, stats=ref.band_stats(bands), sigma=ref.estimate_sigma(bands, True), sigma_all=ref.estimate_sigma(bands, False))
            for a in bands + [r["stats"], r["sigma"], r["sigma_all"]]:
                a.setflags(write=False)
            _REF[key] = r
        self.ref = _REF[key]

    def bands(self):
        return [self.W.coeff_only(num) for num in range(self.nbands)]

    def set_bands(self, bands):
        for num, b in enumerate(bands):
            self.W.set_coeff(np.ascontiguousarray(b), num)

    def intermediates(self):
        """A_l of every level below the last, out of the level's arena: the depth half in front of 'daa'."""
        out = []
        for l in range(1, self.W.levels):
            num = volume_ref.num_of(l, "daa")
            shp = self.W.band_shape(num)
            n = int(np.prod(shp))
            addr = self.W._addr(self.W.coeff_device(num)) - n * np.dtype(self.dtype).itemsize
            out.append(self.W._read(addr, shp, self.dtype))
        return out

    def state(self):
        return self.W.info()["state"]


def assert_bands(got, want, what):
    for num, (g, r) in enumerate(zip(got, want)):
        assert sparsify_ref.same_bits(g, r), (what, num)


def assert_same_arrays(got, want, what):
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        assert sparsify_ref.same_bits(g, r), (what, i)


# ------------------------------------------------------------------------------------------------------------ band_stats, norms
@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_band_stats_and_norms_device(case, dtype):
    v = Vol(case, dtype)
    view = v.W.band_stats()
    assert view.shape == (v.nbands, 2) and view.dtype == np.float64
    got = v.W.read_band_stats(view)
    again = v.W.read_band_stats(v.W.band_stats())
    assert got.tobytes() == again.tobytes()
    want = v.ref["stats"]
    worst = 0.0
    for num in range(v.nbands):
        bound = 2.0 * v.ref["bands"][num].size * 2.0 ** -53
        for k in range(2):
            err = abs(got[num, k] - want[num, k])
            worst = max(worst, err / want[num, k] / bound)
            assert err <= bound * want[num, k], (num, k, got[num, k], want[num, k])
    print("band_stats %s: worst error %.3f of the bound" % (IDS[PARAMS.index((case, dtype))], worst))
    nview = v.W.norms_device()
    assert nview.shape == (2,) and nview.dtype == np.float64
    n1, n2 = v.W.read_norms(nview)
    assert (n1, n2) == v.W.read_norms()
    rel = 2.0 * sum(b.size for b in v.ref["bands"]) * 2.0 ** -53
    assert abs(got[:, 0].sum() - n1) <= rel * n1 and abs(got[:, 1].sum() - n2) <= rel * n2
    m1, m2 = v.W.norms()  # the blocking entry point, unchanged
    assert abs(m1 - n1) <= rel * n1 and abs(m2 - n2) <= rel * n2
    out = DevBuf(np.zeros((v.nbands, 2)))
    assert v.W.band_stats(out=out) is out
    assert v.W.read_band_stats(out).tobytes() == got.tobytes()
    out2 = DevBuf(np.zeros(2))
    assert v.W.norms_device(out=out2) is out2
    assert v.W.read_norms(out2) == (n1, n2)


# -------------------------------------------------------------------------------------------------------------- estimate_sigma
@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_estimate_sigma_is_exact(case, dtype):
    v = Vol(case, dtype)
    view = v.W.estimate_sigma()
    assert view.shape == (1,) and view.dtype == np.float64
    got = v.W.read_sigma(view)
    assert np.array_equal(got, v.ref["sigma"]), (got, v.ref["sigma"])
    got = v.W.read_sigma(v.W.estimate_sigma(skip_zeros=False))
    assert np.array_equal(got, v.ref["sigma_all"]), (got, v.ref["sigma_all"])
    out = DevBuf(np.zeros(1))
    assert v.W.estimate_sigma(out=out) is out
    assert np.array_equal(v.W.read_sigma(out), v.ref["sigma"])


@pytest.mark.parametrize("case,dtype", [PARAMS[1], PARAMS[4], PARAMS[6]], ids=[IDS[1], IDS[4], IDS[6]])
def test_estimate_sigma_on_injected_values(case, dtype):
    """The noise band set to signed zeros, denormals, +-max, +-inf, a NaN and ties (ops_ref.edge_vector), to small integers of
    which a third are zeros, and to nearly nothing but zeros; the other sub-bands keep their values and must not matter."""
    v = Vol(case, dtype)
    shp = v.W.band_shape(ref.NOISE_BAND)
    n = int(np.prod(shp))
    rng = np.random.default_rng(7)
    for kind in range(4):
        if kind == 0:
            x = ops_ref.tile(ops_ref.edge_vector(2.5, dtype, seed=5), n)
        elif kind == 1:
            x = rng.integers(-3, 4, n).astype(dtype)
            x[::5] = -0.0
        else:
            x = np.zeros(n, dtype=dtype)
            x[:kind] = 4.0
        band = rng.permutation(x).reshape(shp)
        v.W.set_coeff(band, ref.NOISE_BAND)
        bands = list(v.ref["bands"])
        bands[ref.NOISE_BAND] = band
        for skip in (True, False):
            got = v.W.read_sigma(v.W.estimate_sigma(skip_zeros=skip))
            want = ref.estimate_sigma(bands, skip)
            assert np.array_equal(got, want, equal_nan=True), (kind, skip, got, want)


# ------------------------------------------------------------------------------------------------------------- threshold_bands
def table_of(v, seed=3):
    rng = np.random.default_rng(seed)
    T = rng.uniform(0.5, 30.0, v.nbands).astype(v.dtype)
    T[v.nbands - 2] = np.nan
    T[1] = 0.0
    return T


@pytest.mark.parametrize("op", ["soft", "hard"])
@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_threshold_bands_bit_identical(case, dtype, op):
    """A table from host and from device memory, with betas[0] set (A_L is thresholded) and with NaN there (it is left alone); a NaN
    entry leaves its sub-band untouched; the intermediates keep their bits; norms() afterwards is the reference's."""
    for where in ("host", "device"):
        for app in (True, False):
            v = Vol(case, dtype)
            bands = v.ref["bands"]
            inter = v.intermediates()
            T = table_of(v)
            if not app:
                T[0] = np.nan
            want = ref.threshold_bands(bands, T, op)
            v.W.threshold_bands(T if where == "host" else DevBuf(T), op)
            assert_bands(v.bands(), want, (where, app))
            assert sparsify_ref.same_bits(v.bands()[v.nbands - 2], bands[v.nbands - 2])
            if not app:
                assert sparsify_ref.same_bits(v.bands()[0], bands[0])
            assert_same_arrays(v.intermediates(), inter, (where, app, "intermediates"))
            n1, n2 = ops_ref.norms(want)
            rel = 2.0 * sum(b.size for b in want) * 2.0 ** -53
            g1, g2 = v.W.norms()
            assert abs(g1 - n1) <= rel * n1 and abs(g2 - n2) <= rel * n2, (g1, n1, g2, n2)
    # the same bits as the global threshold with that value
    v, u = Vol(case, dtype), Vol(case, dtype)
    v.W.threshold_bands(np.full(v.nbands, 7.5, dtype=dtype), op)
    getattr(u.W, op + "_threshold")(7.5, do_threshold_appcoeffs=1)
    assert_bands(v.bands(), u.bands(), "global")
    with pytest.raises(ValueError):
        v.W.threshold_bands(np.zeros(v.nbands + 1, dtype=dtype))
    with pytest.raises(ValueError):
        v.W.threshold_bands(np.zeros(v.nbands, dtype=dtype), "firm")


# --------------------------------------------------------------------------------------------------------------------- denoise
def check_table(v, sigma, got_T, method):
    """tests/test_gpu_adaptive.py's check_table for the sub-bands of a volume."""
    dt = np.dtype(v.dtype)
    bands, stats = v.ref["bands"], v.ref["stats"]
    want_T = ref.threshold_table(bands, sigma, method, v.shape, stats=stats)
    assert np.isnan(got_T[0]) and got_T.dtype == dt and got_T.shape == (v.nbands,)
    rounding = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    eps = float(np.finfo(dt).eps)
    left_out, worst = 0, 0.0
    for num in range(1, v.nbands):
        n = bands[num].size
        g, r = float(got_T[num]), float(want_T[num])
        if method == "VisuShrink":
            assert abs(g - r) <= 2 * rounding * abs(r), (num, g, r)
            continue
        var = sigma[0] * sigma[0]
        m = stats[num, 1] / n
        if abs(m - var - eps) < 2.0 * n * 2.0 ** -53 * m:
            left_out += 1
            continue
        A = m / abs(m - var)
        bound = rounding + A * n * 2.0 ** -52
        worst = max(worst, abs(g - r) / abs(r) / bound)
        assert abs(g - r) <= bound * abs(r), (num, g, r, A, n)
    assert left_out <= 1, left_out
    print("denoise table %s %s: worst %.3g of the bound, %d left out" % (IDS[PARAMS.index((v.case, v.dtype))], method, worst, left_out))


@pytest.mark.parametrize("method,op", [("BayesShrink", "soft"), ("VisuShrink", "hard")])
@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_denoise_in_two_steps(case, dtype, method, op):
    """First the table of last_thresholds() against the reference's, then the coefficients: bit-identical to the reference sweep
    applied with the DEVICE's table; the intermediates keep their bits."""
    v = Vol(case, dtype)
    inter = v.intermediates()
    v.W.denoise(method=method, mode=op)
    sigma, T = v.W.last_thresholds()
    assert sigma.shape == (1,) and np.array_equal(sigma, v.ref["sigma"]), (sigma, v.ref["sigma"])
    check_table(v, sigma, T, method)
    assert_bands(v.bands(), ref.threshold_bands(v.ref["bands"], T, op), method)
    assert_same_arrays(v.intermediates(), inter, "intermediates")


@pytest.mark.parametrize("case,dtype", [PARAMS[0], PARAMS[7]], ids=[IDS[0], IDS[7]])
def test_denoise_with_a_given_sigma(case, dtype):
    v = Vol(case, dtype)
    v.W.denoise(sigma=17.25)
    sigma, T = v.W.last_thresholds()
    assert np.array_equal(sigma, [17.25])
    check_table(v, sigma, T, "BayesShrink")
    assert_bands(v.bands(), ref.threshold_bands(v.ref["bands"], T, "soft"), "given sigma")
    v = Vol(case, dtype)
    v.W.denoise(method="VisuShrink", skip_zeros=False)
    assert np.array_equal(v.W.last_thresholds()[0], v.ref["sigma_all"])
    with pytest.raises(ValueError):
        v.W.denoise(sigma=[1.0, 2.0])
    with pytest.raises(ValueError):
        v.W.denoise(method="SureShrink")


def test_denoise_lowers_the_error_end_to_end():
    case = CASES[3]
    from pypwt_amd import Wavelets3D
    clean, noisy = clean_of(case[0]), noisy_of(case).astype(np.float32)
    W = Wavelets3D(noisy, case[1], case[2])
    W.forward()
    W.denoise()
    W.inverse()
    before = float(np.mean((noisy.astype(np.float64) - clean) ** 2))
    after = float(np.mean((W.image.astype(np.float64) - clean) ** 2))
    print("MSE against the clean pattern: %.4g -> %.4g" % (before, after))
    assert after < before


# --------------------------------------------------------------------------------------------- select_magnitude, keep_largest
@pytest.mark.parametrize("case,dtype", PARAMS, ids=IDS)
def test_select_and_keep_on_own_coefficients(case, dtype):
    v = Vol(case, dtype)
    bands = v.ref["bands"]
    inter = v.intermediates()
    for do_app in (0, 1):
        n = ref.count(bands, do_app)
        assert n == v.W._sparsify_count(do_app)
        for k in (0, 1, n // 3, n - 1, n, n + 5):
            thr, kept, want = ref.keep_largest(bands, k, do_app)
            t_view, k_view = v.W.select_magnitude(k, do_threshold_appcoeffs=do_app)
            assert t_view.shape == (1,) and t_view.dtype == np.dtype(dtype) and k_view.shape == (1,) and k_view.dtype == np.uint64
            got_t, got_kept = v.W.last_sparsify()
            assert sparsify_ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept), ("select", do_app, k, got_t, thr, got_kept, kept)
            assert_bands(v.bands(), bands, ("select is read-only", do_app, k))
            v.W.keep_largest(k, do_threshold_appcoeffs=do_app)
            got_t, got_kept = v.W.last_sparsify()
            assert sparsify_ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept), ("keep", do_app, k, got_t, thr, got_kept, kept)
            got = v.bands()
            assert_bands(got, want, (do_app, k))
            if not do_app:
                assert sparsify_ref.same_bits(got[0], bands[0])
            assert_same_arrays(v.intermediates(), inter, (do_app, k, "intermediates"))
            v.set_bands(bands)
    # a fraction is K = round(fraction * N) from the band shapes
    n = ref.count(bands, 0)
    v.W.keep_largest(fraction=0.25)
    thr, kept, want = ref.keep_largest(bands, int(round(0.25 * n)), 0)
    got_t, got_kept = v.W.last_sparsify()
    assert sparsify_ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept)
    assert_bands(v.bands(), want, "fraction")


def injected(dtype, shapes, seed):
    """Small integers with many ties, zeros and -0.0, denormals, and in the last sub-band one NaN and +-inf."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    bands = []
    for num, shape in enumerate(shapes):
        flat = rng.integers(-3, 4, int(np.prod(shape))).astype(dt)
        flat[::7] = -0.0
        flat[1::11] = fi.smallest_subnormal
        flat[2::13] = -np.nextafter(fi.tiny, dt(0))
        if num == len(shapes) - 1:
            flat[5] = np.nan
            flat[9] = np.inf
            flat[17] = -np.inf
        bands.append(flat.reshape(shape))
    return bands


@pytest.mark.parametrize("case,dtype", [PARAMS[1], PARAMS[2], PARAMS[7]], ids=[IDS[1], IDS[2], IDS[7]])
def test_injected_ties_nan_inf_denormals(case, dtype):
    v = Vol(case, dtype)
    bands = injected(dtype, [b.shape for b in v.ref["bands"]], 13)
    for do_app in (0, 1):
        n = ref.count(bands, do_app)
        allk = np.concatenate([sparsify_ref.keys(bands[b]).ravel() for b in range(0 if do_app else 1, len(bands))])
        at_least = lambda x: int(np.count_nonzero(allk >= sparsify_ref.keys(np.array([x], dtype=dtype))[0]))
        sub = np.finfo(dtype).smallest_subnormal
        # K = 1: the NaN is the threshold; 2: the infinities tie; inside and at both ends of the ties at 3, 2, 1, the denormals, 0
        for k in [1, 2, 3, at_least(3.0) - 1, at_least(3.0), at_least(3.0) + 1, at_least(2.0) - 1, at_least(1.0) + 1, at_least(sub),
                  at_least(sub) + 1, n - 1]:
            v.set_bands(bands)
            v.W.keep_largest(k, do_threshold_appcoeffs=do_app)
            thr, kept, want = ref.keep_largest(bands, k, do_app)
            got_t, got_kept = v.W.last_sparsify()
            assert sparsify_ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept), (do_app, k, got_t, thr, got_kept, kept)
            assert_bands(v.bands(), want, (do_app, k))
            if k == 1:
                assert np.isnan(got_t[0]) and got_kept[0] == 1
            if k == 2:
                assert np.isposinf(got_t[0]) and got_kept[0] == 3
            if k == at_least(3.0) - 1:
                assert got_t[0] == 3 and got_kept[0] == at_least(3.0) > k  # a tie boundary: more than K survive
            v.set_bands(bands)
            v.W.select_magnitude(k, do_threshold_appcoeffs=do_app)
            got_t, got_kept = v.W.last_sparsify()
            assert sparsify_ref.same_bits(got_t, thr) and np.array_equal(got_kept, kept)


def test_bad_arguments():
    v = Vol(CASES[0], np.float32)
    for kw in (dict(), dict(k=1, fraction=0.5), dict(k=-1), dict(k=1.5), dict(k=[1, 2]), dict(fraction=1.5), dict(fraction=float("nan")),
               dict(fraction="half")):
        with pytest.raises(ValueError):
            v.W.select_magnitude(**kw)
        with pytest.raises(ValueError):
            v.W.keep_largest(**kw)
    from pypwt_amd import _lib
    lib = v.W._lib
    assert lib.pdwt_volume_select_magnitude_async(v.W._h, -1, 0, None, None) == _lib.ERR_ARG
    assert lib.pdwt_volume_keep_largest_async(v.W._h, -1, 0) == _lib.ERR_ARG
    assert lib.pdwt_volume_threshold_bands(v.W._h, 0, None, 0) == _lib.ERR_ARG
    assert lib.pdwt_volume_denoise_async(v.W._h, 7, 0, None, 1) == _lib.ERR_ARG
    assert_bands(v.bands(), v.ref["bands"], "nothing was done")


# ----------------------------------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_after_inverse_the_sweeps_warn_and_the_readers_refuse(dtype, capsys):
    from pypwt_amd import _lib
    v = Vol(CASES[3], dtype)
    v.W.denoise()
    before = v.W.last_thresholds()
    v.W.keep_largest(100)
    sp = v.W.last_sparsify()
    v.W.inverse()
    img, st = v.W.image, v.state()
    capsys.readouterr()
    v.W.threshold_bands(np.full(v.nbands, 5.0, dtype=dtype))
    v.W.denoise(method="VisuShrink")
    v.W.keep_largest(10)
    out = capsys.readouterr().out
    assert out.count("Warning") == 3 and out.count("modified by inverse()") == 3
    assert np.array_equal(v.W.image, img) and v.state() == st
    after = v.W.last_thresholds()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    assert all(np.array_equal(a, b) for a, b in zip(sp, v.W.last_sparsify()))
    lib, h = v.W._lib, v.W._h
    assert lib.pdwt_volume_band_stats_async(h, None) == _lib.ERR_STATE
    assert lib.pdwt_volume_norms_async(h, None) == _lib.ERR_STATE
    assert lib.pdwt_volume_estimate_sigma_async(h, 1, None) == _lib.ERR_STATE
    assert lib.pdwt_volume_select_magnitude_async(h, 5, 0, None, None) == _lib.ERR_STATE
    with pytest.raises(_lib.PdwtError):
        v.W.band_stats()
    # forward() makes the coefficients current again
    v.W.forward()
    assert np.isfinite(v.W.read_sigma(v.W.estimate_sigma())).all()
