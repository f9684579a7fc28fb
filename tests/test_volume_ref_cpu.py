"""The 3D reference of the volume tests and the host half of the pdwt_volume_* ABI, without a GPU.

1. tests/volume_ref.py -- the 3D DWT as a composition of the CPU oracle -- equals pywt.wavedecn(mode="periodization") as
   recorded in tests/golden/volume.npz (tests/golden/make_volume_golden.py): shapes, keys, values.  Bound: 2e-6 relative to the
   scale of the data.
2. pdwt_volume_layout, a pure host function of the library, equals the composition's shapes and level clamp over a sweep of sizes.
3. pdwt_volume_create refuses bad arguments before it looks for a device, and fails with PDWT_ERR_HIP -- no crash -- where
   there is none.
"""
import ctypes as C
import os

import numpy as np
import pytest

import volume_ref
from pypwt_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volume.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_file_is_what_the_generator_describes(golden):
    assert list(golden["cases"]) == ["c0", "c1", "c2", "c3"]
    want = {"c0": ((9, 10, 13), "db2", 1), "c1": ((7, 5, 6), "haar", 2), "c2": ((16, 12, 20), "sym4", 1), "c3": ((20, 24, 28), "db2", 2)}
    for c, (shape, w, lv) in want.items():
        assert golden[c + "_x"].shape == shape and golden[c + "_x"].dtype == np.float64
        assert str(golden[c + "_wname"]) == w and int(golden[c + "_levels"]) == lv
    assert os.path.getsize(GOLDEN) < 512 * 1024
    assert any(str(v).startswith("pywt ") for v in golden["versions"])


@pytest.mark.parametrize("case", ["c0", "c1", "c2", "c3"])
@pytest.mark.parametrize("double", [False, True, "full"])
def test_composition_equals_pywt(golden, case, double):
    x = golden[case + "_x"]
    w, lv = str(golden[case + "_wname"]), int(golden[case + "_levels"])
    assert volume_ref.clamp_levels(x.shape, volume_ref.hlen_of(w), lv) == lv
    bands = volume_ref.forward(x, w, lv, double=double)
    shapes = volume_ref.band_shapes(x.shape, lv)
    assert len(bands) == 1 + 7 * lv == len(shapes)
    tol = 2e-6 * float(np.abs(x).max())
    want = [golden[case + "_a"]] + [golden["%s_l%d_%s" % (case, l, k)] for l in range(1, lv + 1) for k in volume_ref.KEYS]
    # the file holds exactly these keys: nothing pywt produced is left out
    assert sum(1 for k in golden.files if k.startswith(case + "_l") and k[len(case) + 2].isdigit()) == 7 * lv
    for num, (b, g) in enumerate(zip(bands, want)):
        assert b.shape == g.shape == shapes[num], (num, b.shape, g.shape)
        err = float(np.abs(b.astype(np.float64) - g).max())
        print(case, double, num, "max abs diff %.3g (bound %.3g)" % (err, tol))
        assert err <= tol, (num, err, tol)
    # pywt's own order out of ours
    dec = volume_ref.to_wavedecn(bands, lv)
    assert len(dec) == lv + 1 and sorted(dec[1]) == list(volume_ref.KEYS)
    assert dec[-1]["ddd"] is bands[volume_ref.num_of(1, "ddd")]
    # and the way back
    back = volume_ref.inverse(bands, x.shape, w, lv, double=double)
    assert back.shape == x.shape
    assert float(np.abs(back.astype(np.float64) - x).max()) <= (2e-6 if double == "full" else 7e-4) * float(np.abs(x).max())


def _layout(lib, shape, wname, levels, cap=None):
    nlev = C.c_int(-1)
    cap = 1 + 7 * 16 if cap is None else cap
    dims = (C.c_int * (3 * max(cap, 1)))()
    n = lib.pdwt_volume_layout(shape[0], shape[1], shape[2], wname.encode(), levels, C.byref(nlev), dims, cap)
    return n, nlev.value, [tuple(dims[3 * k:3 * k + 3]) for k in range(max(min(n, cap), 0))]


@pytest.mark.parametrize("variant", ["f32", "f64"])
def test_layout_equals_the_composition(variant):
    lib = _lib.load(variant)
    sizes = [2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 69, 70]
    rng = np.random.default_rng(5)
    shapes = [(a, b, c) for a in (2, 3, 8, 9, 70) for b in (2, 5, 16, 33) for c in (2, 7, 64, 69)]
    shapes += [tuple(int(s) for s in rng.choice(sizes, 3)) for _ in range(60)]
    shapes += [(n, n, n) for n in range(2, 71)]
    for wname in ("haar", "db2", "db4", "sym8", "db20"):
        hlen = volume_ref.hlen_of(wname)
        for shape in shapes:
            for levels in (0, 1, 2, 3, 9):
                n, nlev, dims = _layout(lib, shape, wname, levels)
                want_lev = volume_ref.clamp_levels(shape, hlen, levels)
                assert nlev == want_lev, (shape, wname, levels, nlev, want_lev)
                assert n == 1 + 7 * want_lev
                assert dims == volume_ref.band_shapes(shape, want_lev), (shape, wname, levels)
    # a short buffer is filled as far as it goes; no buffer at all is allowed
    n, nlev, dims = _layout(lib, (64, 64, 64), "haar", 3, cap=5)
    assert (n, nlev) == (22, 3) and dims == volume_ref.band_shapes((64, 64, 64), 3)[:5]
    assert lib.pdwt_volume_layout(64, 64, 64, b"haar", 3, None, None, 0) == 22


def test_layout_and_create_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    h = _lib.handle_t()
    img = np.zeros((4, 4, 4), dtype=np.float32)
    p = img.ctypes.data_as(C.c_void_p)
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, 4, -3), (65535, 4, 4), (1 << 20, 2, 2)):
        assert lib.pdwt_volume_create(p, shape[0], shape[1], shape[2], b"haar", 1, 1, -1, None, C.byref(h)) == _lib.ERR_ARG, shape
        assert not h.value
        assert _lib.last_error(lib)
        assert lib.pdwt_volume_layout(shape[0], shape[1], shape[2], b"haar", 1, None, None, 0) == _lib.ERR_ARG
    assert lib.pdwt_volume_layout(65534, 2, 2, b"haar", 1, None, None, 0) == 8  # the largest depth is accepted
    assert lib.pdwt_volume_create(p, 4, 4, 4, b"no_such_wavelet", 1, 1, -1, None, C.byref(h)) == _lib.ERR_WAVELET
    assert lib.pdwt_volume_layout(4, 4, 4, b"no_such_wavelet", 1, None, None, 0) == _lib.ERR_WAVELET
    assert lib.pdwt_volume_create(p, 4, 4, 4, None, 1, 1, -1, None, C.byref(h)) == _lib.ERR_ARG
    assert lib.pdwt_volume_create(p, 4, 4, 4, b"haar", 1, 1, -1, None, None) == _lib.ERR_ARG
    # null handles are answered, not dereferenced
    assert lib.pdwt_volume_forward(None) == _lib.ERR_ARG and lib.pdwt_volume_inverse(None) == _lib.ERR_ARG
    assert lib.pdwt_volume_destroy(None) == _lib.OK
    assert lib.pdwt_volume_image_ptr(None) == 0 and lib.pdwt_volume_coeff_ptr(None, 0) == 0
    assert lib.pdwt_volume_stream(None) is None


def test_create_fails_with_err_hip_where_there_is_no_device():
    lib = _lib.load()
    if lib.pdwt_device_count() > 0:
        return  # a HIP device is present: tests/test_gpu_volume.py covers creation
    h = _lib.handle_t()
    img = np.zeros((4, 6, 8), dtype=np.float32)
    rc = lib.pdwt_volume_create(img.ctypes.data_as(C.c_void_p), 4, 6, 8, b"db2", 1, 1, -1, None, C.byref(h))
    assert rc == _lib.ERR_HIP and not h.value
    assert "no HIP device" in _lib.last_error(lib)
    import pypwt_amd
    with pytest.raises(_lib.PdwtError):
        pypwt_amd.Wavelets3D(img, "db2", 1)
    with pytest.raises(ValueError):
        pypwt_amd.Wavelets3D(img[0], "db2", 1)  # two dimensions
    with pytest.raises(ValueError):
        pypwt_amd.Wavelets3D(img.astype(np.float64), "db2", 1)  # wrong dtype for the fp32 class
