"""tests/sparsify_ref.py (the rule the GPU tests compare against) pinned to np.partition on tie-free data and to hand-written
tie, NaN, inf and signed-zero cases."""
import numpy as np
import pytest

import sparsify_ref as ref


def bands_of(detail, app=None):
    """[approximation, one detail band] of one image out of flat lists."""
    detail = np.asarray(detail)
    app = np.zeros(1, dtype=detail.dtype) if app is None else np.asarray(app, dtype=detail.dtype)
    return [app.reshape(1, 1, -1), detail.reshape(1, 1, -1)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tie_free_data_equals_partition(dtype):
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 1000):
        x = rng.permutation(np.arange(1, n + 1)).astype(dtype) * rng.choice([-1, 1], n).astype(dtype) * dtype(0.37)
        for k in sorted({1, 2, n // 3, n - 1} - {0, n}):
            want = np.partition(np.abs(x), n - k)[n - k]
            thr, kept, out = ref.keep_largest(bands_of(x), k)
            assert thr[0] == want and thr.dtype == dtype
            assert kept[0] == k
            assert np.array_equal(out[1].ravel(), np.where(np.abs(x) >= want, x, 0))
            assert np.count_nonzero(out[1]) == k
            t2, k2 = ref.select_magnitude(bands_of(x), k)
            assert t2[0] == thr[0] and k2[0] == kept[0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_two_ends(dtype):
    x = np.array([3, -1, 2, -0.0, 5], dtype=dtype)
    thr, kept, out = ref.keep_largest(bands_of(x), 0)
    assert np.isposinf(thr[0]) and kept[0] == 0
    assert ref.same_bits(out[1].ravel(), np.zeros(5, dtype=dtype))  # -0.0 became +0.0 too
    for k in (5, 6, 10 ** 12):
        thr, kept, out = ref.keep_largest(bands_of(x), k)
        assert thr[0] == 0 and kept[0] == 5
        assert ref.same_bits(out[1].ravel(), x)  # -0.0 kept as it is
    thr, kept, _ = ref.keep_largest(bands_of(x), -3)
    assert np.isposinf(thr[0]) and kept[0] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ties_all_survive(dtype):
    x = np.array([1, -2, 2, 2, -2, 3, -3, 9, 0, -0.0], dtype=dtype)
    # sorted magnitudes: 0 0 1 2 2 2 2 3 3 9
    for k, t, kept in ((1, 9, 1), (2, 3, 3), (3, 3, 3), (4, 2, 7), (7, 2, 7), (8, 1, 8), (9, 0, 10)):
        thr, cnt, out = ref.keep_largest(bands_of(x), k)
        assert (thr[0], cnt[0]) == (t, kept), k
        assert ref.same_bits(out[1].ravel(), np.where(np.abs(x) >= t, x, dtype(0)))
    # K = 9: the threshold is a zero, every element is "at least as large": nothing changes, -0.0 stays -0.0
    assert ref.same_bits(ref.keep_largest(bands_of(x), 9)[2][1].ravel(), x)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_orders_behind_inf(dtype):
    x = np.array([1, -np.inf, np.nan, 2, np.inf, -3], dtype=dtype)
    thr, kept, out = ref.keep_largest(bands_of(x), 1)
    assert np.isnan(thr[0]) and kept[0] == 1
    assert ref.same_bits(out[1].ravel(), np.array([0, 0, np.nan, 0, 0, 0], dtype=dtype))
    thr, kept, out = ref.keep_largest(bands_of(x), 2)
    assert np.isposinf(thr[0]) and kept[0] == 3  # the two infinities tie
    assert ref.same_bits(out[1].ravel(), np.array([0, -np.inf, np.nan, 0, np.inf, 0], dtype=dtype))
    thr, kept, _ = ref.keep_largest(bands_of(x), 4)
    assert thr[0] == 3 and kept[0] == 4
    # a negative NaN has the key of the positive one with the same payload
    y = np.array([1.0, -np.nan], dtype=dtype)
    assert ref.keys(y)[1] == ref.keys(np.abs(y))[1] and ref.keys(y)[1] > ref.keys(np.array([np.inf], dtype=dtype))[0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_approximation_joins_only_when_asked(dtype):
    det = np.array([1, 2, 3, 4], dtype=dtype)
    app = np.array([100, 0.5], dtype=dtype)
    thr, kept, out = ref.keep_largest(bands_of(det, app), 2, do_app=0)
    assert thr[0] == 3 and kept[0] == 2 and ref.same_bits(out[0].ravel(), app)
    assert ref.count(bands_of(det, app), 0) == 4 and ref.count(bands_of(det, app), 1) == 6
    thr, kept, out = ref.keep_largest(bands_of(det, app), 2, do_app=1)
    assert thr[0] == 4 and kept[0] == 2
    assert np.array_equal(out[0].ravel(), [100, 0]) and np.array_equal(out[1].ravel(), [0, 0, 0, 4])


def test_one_k_per_image():
    b = [np.zeros((2, 1, 1), dtype=np.float32), np.array([[[1, 2, 3]], [[-6, 5, 4]]], dtype=np.float32)]
    thr, kept, out = ref.keep_largest(b, [1, 2])
    assert list(thr) == [3, 5] and list(kept) == [1, 2]
    assert np.array_equal(out[1], np.array([[[0, 0, 3]], [[-6, 5, 0]]], dtype=np.float32))
    thr, kept = ref.select_magnitude(b, 3)
    assert list(thr) == [0, 0] and list(kept) == [3, 3]
