"""The numpy references of tests/ops_ref.py against the committed C oracle (oracle/pdwt_oracle.c), float32, BIT FOR BIT: every
operator, do_app and normalize in {0, 1}, beta in {7.5, 0, -1.0}, on an odd 2D DWT, a 2D SWT and a 1D plan, on transform
coefficients and on the vector of edge values (signed zeros, +-beta and its neighbours, denormals, max, infinities, NaN).
This is what lets the GPU tests of the operators use numpy where the oracle's wrapper does not reach (fp64, batches, 2^24 values).
No GPU needed."""
import math

import numpy as np
import pytest

import ops_ref
from oracle import oracle

# (shape, ndim, do_swt, wavelet, levels)
PLANS = [((61, 59), 2, 0, "db2", 3), ((40, 52), 2, 1, "haar", 3), ((1, 301), 1, 0, "sym4", 4), ((5, 128), 1, 1, "db2", 2)]
BETAS = [7.5, 0.0, -1.0]


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle.build()


def _bands(plan, kind, beta):
    shape, nd, swt, wname, lv = plan
    x = oracle.hash_input(shape, 17, 100.0) - 50.0
    bands = oracle.forward(x, wname, lv, ndim=nd, do_swt=swt)
    if kind == "edge":
        vec = ops_ref.edge_vector(beta if beta else 7.5, np.float32)
        bands = [ops_ref.tile(np.roll(vec, k), b.size).reshape(b.shape) for k, b in enumerate(bands)]
    return [np.ascontiguousarray(b, dtype=np.float32) for b in bands]


def _same(got, ref):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert ops_ref.same_bits(np.asarray(g).reshape(r.shape), r), "band %d" % k


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("kind", ["coeffs", "edge"])
@pytest.mark.parametrize("beta", BETAS)
def test_elementwise_references_equal_the_oracle_bit_for_bit(plan, kind, beta):
    shape, nd, swt, wname, lv = plan
    bands = _bands(plan, kind, beta)
    for op in ("soft", "hard", "linf"):
        for do_app in (0, 1):
            for normalize in (0, 1):
                ref = oracle.threshold(bands, shape, lv, op, beta, do_app, normalize, ndim=nd, do_swt=swt)
                _same(ops_ref.threshold(bands, lv, nd, op, beta, do_app, normalize), ref)
    for do_app in (0, 1):
        if beta == -1.0:
            continue  # 1 / (1 + beta) divides by zero: left out, here and in the GPU tests
        _same(ops_ref.shrink(bands, beta, do_app), oracle.shrink(bands, shape, lv, beta, do_app, ndim=nd, do_swt=swt))


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("beta", [20.0, 0.0])
def test_group_soft_reference_is_the_oracle_within_its_float32_rounding(plan, beta):
    """The oracle runs the chain (three squares, sum, sqrt, division, subtraction, product) in float32, the reference in float64
    rounded once: a handful of float32 roundings of values of the size of the band apart, 5e-6 * max|band| as in the GPU tests."""
    shape, nd, swt, wname, lv = plan
    bands = _bands(plan, "coeffs", beta)
    for do_app in (0, 1):
        if do_app and not swt:
            continue  # the approximation band has the detail shape only for the SWT
        for normalize in (0, 1):
            ref = oracle.threshold(bands, shape, lv, "group", beta, do_app, normalize, ndim=nd, do_swt=swt)
            got, _ = ops_ref.group_soft(bands, lv, nd, beta, do_app, normalize)
            for g, r in zip(got, ref):
                assert np.abs(g - r).max() <= 5e-6 * max(np.abs(r).max(), 1.0)


@pytest.mark.parametrize("plan", PLANS)
def test_norms_and_axpy_references(plan):
    shape, nd, swt, wname, lv = plan
    bands = _bands(plan, "coeffs", 7.5)
    n1, n2 = ops_ref.norms(bands)
    o1, o2 = oracle.norms(bands, shape, lv, ndim=nd, do_swt=swt)  # recursive float64 sums: (n - 1) * 2^-53 of the sum
    n = sum(b.size for b in bands)
    assert abs(n1 - o1) <= n * 2.0 ** -53 * n1 and abs(n2 - o2) <= n * 2.0 ** -53 * n2
    flat = np.concatenate([b.ravel() for b in bands]).astype(np.float64)
    assert n1 == math.fsum(np.abs(flat)) and n2 == math.fsum(flat * flat)
    other = [np.roll(b, 1) for b in bands]
    got = ops_ref.axpy(bands, other, 0.5)
    for g, a, b in zip(got, bands, other):
        assert g.dtype == np.float32 and np.array_equal(g, (a.astype(np.float64) + 0.5 * b.astype(np.float64)).astype(np.float32))


def test_level_betas_round_to_the_band_type_after_every_step():
    b32 = ops_ref.level_betas(7.5, 5, 1, np.float32)
    b = np.float32(7.5)
    for l in range(5):
        b = np.float32(np.float64(b) / 1.4142135623730951)
        assert b32[l] == b and type(b32[l]) is np.float32
    assert ops_ref.level_betas(7.5, 3, 0, np.float64) == [7.5, 7.5, 7.5]
    assert ops_ref.app_beta(7.5, 4, 1, np.float32) == np.float32(7.5 / 4)
    assert ops_ref.app_beta(7.5, 5, 1, np.float32) == np.float32(np.float64(np.float32(7.5 / 4)) / 1.4142135623730951)
    assert ops_ref.app_beta(7.5, 5, 0, np.float64) == 7.5


def test_edge_vector_holds_what_it_says():
    for dt in (np.float32, np.float64):
        v = ops_ref.edge_vector(7.5, dt)
        fi = np.finfo(dt)
        assert v.dtype == dt and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
        for want in (7.5, -7.5, fi.tiny, fi.max, -fi.max, fi.smallest_subnormal, np.nextafter(dt(7.5), dt(0)), np.nextafter(dt(7.5), dt(np.inf))):
            assert (v == want).any()
        assert np.signbit(v[v == 0]).sum() == 1 and (v == 0).sum() == 2
        assert np.isfinite(ops_ref.edge_vector(7.5, dt, finite_only=True)).all()
        assert ops_ref.tile(v, 1000).size == 1000
