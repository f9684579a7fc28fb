"""The proximal operators of volumes on the GPU -- `group_soft_threshold`, `group_norm`, `proj_linf`, `shrink`, `add_wavelet` of
`Wavelets3D` / `Wavelets3D64`, decimated and stationary -- against tests/volume_prox_ref.py, which tests/test_volume_prox_ref_cpu.py
pins.  The shapes are those of tests/test_emu_volume_group.py: n_l = 3, 1, 2, 0 (mod 4), a tiny one, several pieces with a ragged
last one, and the stationary layout.

In every case the starting coefficients are read back from the device after forward() and the reference is applied to THOSE: the
transform's own error is not in the comparison.

Bounds:
  * group_soft_threshold, per sub-band: fp32 5e-6 max(|ref band|, 1), the project's bound (tests/test_gpu_ops_scale.py, B2); fp64
    8 * 2^-52 max(|ref band|, 1): the sum of up to eight squares, sqrt, division, subtraction and product are about six half-ulp
    roundings, the bound is twice that (the 2D figure was measured on groups of three and does not carry over).  Measured on the
    MI355X, largest error over bound: 0.36 in fp32 and 0.22 in fp64, both on 8 x 8 x 8 haar stationary (the plain fp64 formula
    1 - beta / ||g|| was at 1.16 there; volume_ops_kernels.hpp: vol_group_res says what the fp64 build does instead);
  * proj_linf, shrink: np.array_equal with the reference in the band's own type;
  * add_wavelet: one ulp of the reference (one fused multiply-add against a sum rounded once);
  * group_norm: 2 n 2^-53 relative to the np.longdouble reference (tests/plan_model.py's bound of the library's norms), n = all
    coefficients; two calls give identical bits;
  * inverse() after an operator -- how a touched intermediate would show --: the reconstruction bounds of tests/test_gpu_volume.py /
    tests/test_gpu_volume_swt.py (fp32: tol32 against the fp64 composition; fp64: 1e-12 max(|ref|, 1)).
"""
import ctypes as C

import numpy as np
import pytest

import ops_ref
import volume_prox_ref as prox
import volume_ref
import volume_swt_ref
from oracle import oracle

pytestmark = pytest.mark.gpu

SCALE = 255.0
# (shape, wavelet, levels asked for, stationary): every shape keeps the levels it asks for
CASES = [((9, 10, 13), "haar", 1, 0), ((6, 6, 10), "db2", 1, 0), ((6, 6, 4), "haar", 1, 0), ((16, 16, 16), "db2", 2, 0),
         ((7, 5, 6), "haar", 2, 0), ((40, 48, 44), "db2", 2, 0),
         ((5, 7, 9), "haar", 2, 1), ((9, 10, 13), "db2", 1, 1), ((3, 3, 5), "haar", 1, 1), ((8, 8, 8), "haar", 3, 1),
         ((24, 24, 28), "db2", 3, 1)]
IDS = ["%dx%dx%d-%s-L%d-%s" % (s + (w, l, "swt" if k else "dwt")) for s, w, l, k in CASES]
DTYPES = [np.float32, np.float64]
SOME = [CASES[0], CASES[5], CASES[6], CASES[10]]
SOME_IDS = [IDS[0], IDS[5], IDS[6], IDS[10]]


@pytest.fixture(scope="module")
def classes():
    oracle.build()
    from pypwt_amd import Wavelets3D, Wavelets3D64
    return {np.float32: Wavelets3D, np.float64: Wavelets3D64}


_X = {}


def volume_of(case, seed=0):
    """Seeded data of one case, made once and shared (read-only)."""
    key = (case, seed)
    if key not in _X:
        shape, _, asked, _ = case
        x = np.random.default_rng(1000 * sum(shape) + asked + 7919 * seed).uniform(0.0, SCALE, shape).astype(np.float32)
        x.setflags(write=False)
        _X[key] = x
    return _X[key]


def make(classes, dtype, case, seed=0):
    shape, wname, asked, swt = case
    W = classes[dtype](volume_of(case, seed).astype(dtype), wname, asked, do_swt=swt)
    assert W.levels == asked, (case, W.levels)
    W.forward()
    return W


def again(W, case, dtype, seed=0):
    """The case's coefficients once more, after an inverse() has overwritten the image."""
    W.forward(volume_of(case, seed).astype(dtype))


def all_bands(W):
    return [W.coeff_only(num) for num in range(W.nbands)]


def band_bound(ref_band, dtype):
    eps = 5e-6 if dtype == np.float32 else 8 * 2.0 ** -52
    return eps * max(float(np.abs(ref_band).max()), 1.0)


def ref_inverse(case, bands, double):
    shape, wname, L, swt = case
    if swt:
        return volume_swt_ref.inverse(bands, wname, L, double)
    return volume_ref.inverse(bands, shape, wname, L, double)


def check_inverse(W, case, dtype, want, what):
    """inverse() against the reference inverse of the operated coefficients `want`."""
    L = case[2]
    W.inverse()
    inv64 = ref_inverse(case, [b.astype(np.float64) for b in want], "full")
    got = W.image
    if dtype == np.float32:
        inv32 = ref_inverse(case, want, False)
        rule = 1.5e-6 * (1 + L) * max(float(np.abs(inv64).max()), 1.0)
        tol = max(rule, 2.0 * float(np.abs(inv32.astype(np.float64) - inv64).max()))
    else:
        tol = 1e-12 * max(float(np.abs(inv64).max()), 1.0)
    err = float(np.abs(got.astype(np.float64) - inv64).max())
    print(what, "inverse err %.3g tol %.3g" % (err, tol))
    assert got.dtype == dtype and err <= tol, (what, err, tol)
    again(W, case, dtype)  # for whoever goes on


def beta_for_half(bands, L, do_app, normalize):
    """A beta at which about half of the groups vanish: the median of ||g|| sqrt(2)^l (the level's own scale under normalize)."""
    scaled = []
    for l, idx in enumerate(prox.groups(L, do_app), 1):
        nrm = np.sqrt(sum(bands[i].astype(np.float64) ** 2 for i in idx))
        scaled.append(nrm.ravel() * (ops_ref.SQRT_2 ** l if normalize else 1.0))
    return float(np.median(np.concatenate(scaled)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_group_soft_threshold(classes, case, dtype):
    L = case[2]
    W = make(classes, dtype, case)
    worst = 0.0
    for do_app in (0, 1):
        for normalize in (0, 1):
            before = all_bands(W)
            beta = beta_for_half(before, L, do_app, normalize)
            frac = prox.zeroed_fraction(before, L, beta, do_app, normalize)
            assert 0.25 <= frac <= 0.75, (case, do_app, normalize, frac)
            want = prox.group_soft(before, L, beta, do_app, normalize)
            W.group_soft_threshold(beta, do_app, normalize)
            after = all_bands(W)
            for num, (g, w) in enumerate(zip(after, want)):
                err = float(np.abs(g.astype(np.longdouble) - w.astype(np.longdouble)).max())
                worst = max(worst, err / band_bound(w, dtype))
                assert g.dtype == dtype and err <= band_bound(w, dtype), (case, do_app, normalize, num, err, band_bound(w, dtype))
            if not do_app:
                assert np.array_equal(after[0], before[0])
            assert all(not np.array_equal(g, b) for g, b in zip(after[1:], before[1:]))  # beta bites in every detail sub-band
            check_inverse(W, case, dtype, after, (case, "group_soft", do_app, normalize))
    print(case, np.dtype(dtype).name, "group_soft_threshold: largest error / bound = %.3g" % worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_proj_linf_and_shrink(classes, case, dtype):
    W = make(classes, dtype, case)
    for do_app in (0, 1):
        before = all_bands(W)
        beta = 0.5 * min(float(np.abs(b).max()) for b in before[1:])  # it clips something in every detail sub-band
        W.proj_linf(beta, do_app)
        after, want = all_bands(W), prox.linf(before, beta, do_app)
        for num, (g, w) in enumerate(zip(after, want)):
            assert g.dtype == w.dtype and np.array_equal(g, w), (case, "proj_linf", do_app, num)
        assert np.array_equal(after[0], before[0]) == (not do_app)
        assert all(not np.array_equal(g, b) for g, b in zip(after[1:], before[1:]))
        check_inverse(W, case, dtype, want, (case, "proj_linf", do_app))
        before = all_bands(W)
        W.shrink(0.25, do_app)
        after, want = all_bands(W), prox.shrink(before, 0.25, do_app)
        for num, (g, w) in enumerate(zip(after, want)):
            assert g.dtype == w.dtype and np.array_equal(g, w), (case, "shrink", do_app, num)
        assert np.array_equal(after[0], before[0]) == (not do_app)
        check_inverse(W, case, dtype, want, (case, "shrink", do_app))
    # the defaults are the reference's: the approximation takes part
    before = all_bands(W)
    W.proj_linf(1.0)
    assert np.array_equal(W.coeff_only(0), ops_ref.linf(before[0], 1.0))
    again(W, case, dtype)
    before = all_bands(W)
    W.shrink(1.0)
    assert np.array_equal(W.coeff_only(0), before[0] * dtype(0.5))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_add_wavelet(classes, case, dtype):
    W1, W2 = make(classes, dtype, case, 0), make(classes, dtype, case, 1)
    src = all_bands(W2)
    for alpha in (0.5, -1.25):
        dst = all_bands(W1)
        W1.add_wavelet(W2, alpha)
        got, want = all_bands(W1), prox.axpy(dst, src, alpha)
        for num, (g, w) in enumerate(zip(got, want)):
            ulps = np.abs(g.astype(np.longdouble) - w.astype(np.longdouble)) / np.spacing(np.abs(w)).astype(np.longdouble)
            assert g.dtype == dtype and float(ulps.max()) <= 1.0, (case, alpha, num, float(ulps.max()))
        assert all(np.array_equal(g, s) for g, s in zip(all_bands(W2), src))  # the source is read only
    check_inverse(W1, case, dtype, got, (case, "add_wavelet"))


def test_add_wavelet_refuses_operands_that_differ(classes):
    case = CASES[3]  # (16, 16, 16) db2 L2, decimated
    shape, wname, asked, _ = case
    x = volume_of(case)
    W = make(classes, np.float32, case)
    before = all_bands(W)
    others = {"shape": classes[np.float32](np.zeros((16, 16, 20), np.float32), wname, asked),
              "name": classes[np.float32](x, "haar", asked),
              "levels": classes[np.float32](x, wname, 1),
              "kind": classes[np.float32](x, wname, asked, do_swt=1),
              "precision": classes[np.float64](x.astype(np.float64), wname, asked)}
    for what, other in others.items():
        other.forward()
        with pytest.raises(ValueError):
            W.add_wavelet(other, 0.5)
        assert all(np.array_equal(g, b) for g, b in zip(all_bands(W), before)), what
    from pypwt_amd import _lib
    assert W._lib.pdwt_volume_add_wavelet(W._h, others["kind"]._h, 0.5) == _lib.ERR_MISMATCH
    with pytest.raises(ValueError):
        W.add_wavelet(before[0], 0.5)
    assert all(np.array_equal(g, b) for g, b in zip(all_bands(W), before))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_group_norm(classes, case, dtype):
    L = case[2]
    W = make(classes, dtype, case)
    lend = classes[np.float64](np.zeros((2, 2, 2)), "haar", 1)  # eight float64 of device memory that this test owns
    bands = all_bands(W)
    n = sum(b.size for b in bands)
    for do_app in (0, 1):
        ref = prox.group_norm(bands, L, do_app)
        got = W.group_norm(do_app)
        rel = float(abs(np.longdouble(got) - ref) / ref)
        print(case, np.dtype(dtype).name, "group_norm do_app", do_app, "rel err %.3g bound %.3g" % (rel, 2 * n * 2.0 ** -53))
        assert rel <= 2 * n * 2.0 ** -53, (case, do_app, got, ref)
        assert W.group_norm(do_app) == got  # the same bits
        view = W.group_norm_device(do_threshold_appcoeffs=do_app)
        assert W._read(W._addr(view), (1,), np.float64)[0] == got
        out = lend.image_device
        assert W.group_norm_device(out, do_app) is out
        W.synchronize()
        assert lend.image.ravel()[0] == got and not lend.image.ravel()[1:].any()
    assert W.group_norm() == W.group_norm(0) < W.group_norm(1)
    assert all(np.array_equal(g, b) for g, b in zip(all_bands(W), bands))  # it reads only
    # the threshold lowers the norm to the reference's value: the two differ by at most the members' own differences
    beta = beta_for_half(bands, L, 0, 0)
    W.group_soft_threshold(beta)
    want = prox.group_soft(bands, L, beta)
    ref = prox.group_norm(want, L)
    slack = sum(b.size * band_bound(b, dtype) for b in want[1:]) + 2 * n * 2.0 ** -53 * float(ref)
    got = W.group_norm()
    assert abs(np.longdouble(got) - ref) <= slack and got < 0.75 * float(prox.group_norm(bands, L)), (case, got, ref, slack)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", SOME, ids=SOME_IDS)
def test_moreau_decomposition_on_the_device(classes, case, dtype):
    """soft(c, beta) + proj_linf(c, beta) = c: three of the operators against each other."""
    W1, W2 = make(classes, dtype, case), make(classes, dtype, case)
    c = all_bands(W1)
    beta = float(np.median(np.abs(np.concatenate([b.ravel() for b in c[1:]]))))
    W1.soft_threshold(beta)
    W2.proj_linf(beta, 0)
    W1.add_wavelet(W2, 1.0)
    for num, (g, w) in enumerate(zip(all_bands(W1), c)):
        if num == 0:
            continue  # (A_L + A_L: the approximation was left alone twice)
        assert np.all(np.abs(g.astype(np.longdouble) - w.astype(np.longdouble)) <= np.spacing(np.abs(w))), (case, num)


@pytest.mark.parametrize("swt", [0, 1])
def test_state(classes, swt, capsys):
    from pypwt_amd import _lib
    case = CASES[10] if swt else CASES[3]
    W, W2 = make(classes, np.float32, case), make(classes, np.float32, case, 1)
    lib = W._lib
    W.inverse()
    img = W.image
    res = C.c_double(3.0)
    assert lib.pdwt_volume_group_soft_threshold(W._h, 1.0, 0, 0) == _lib.ERR_STATE
    assert lib.pdwt_volume_proj_linf(W._h, 1.0, 1) == _lib.ERR_STATE
    assert lib.pdwt_volume_shrink(W._h, 1.0, 1) == _lib.ERR_STATE
    assert lib.pdwt_volume_add_wavelet(W._h, W2._h, 1.0) == _lib.ERR_STATE
    assert lib.pdwt_volume_add_wavelet(W2._h, W._h, 1.0) == _lib.ERR_STATE
    assert lib.pdwt_volume_group_norm(W._h, 0, C.byref(res)) == _lib.ERR_STATE and res.value == 3.0
    assert lib.pdwt_volume_group_norm_async(W._h, 0, None, None) == _lib.ERR_STATE
    assert W.info()["state"] == _lib.STATE_INVERSE and np.array_equal(W.image, img)
    capsys.readouterr()
    W.group_soft_threshold(1.0), W.proj_linf(1.0), W.shrink(1.0), W.add_wavelet(W2)  # Python: the warning of soft_threshold
    assert capsys.readouterr().out.count("Warning") == 4
    assert W.info()["state"] == _lib.STATE_INVERSE and np.array_equal(W.image, img)
    W.forward()  # and everything works again
    before = all_bands(W)
    W.group_soft_threshold(5.0, 1, 1)
    W.proj_linf(50.0)
    W.shrink(0.5)
    W.add_wavelet(W2, 0.25)
    assert W.group_norm(1) > 0 and W._read(W._addr(W.group_norm_device()), (1,), np.float64)[0] == W.group_norm()
    assert all(not np.array_equal(g, b) for g, b in zip(all_bands(W), before))
    if swt:  # what stationary volumes refuse stays refused
        with pytest.raises(NotImplementedError, match="denoise"):
            W.denoise()
    W.inverse()
