"""The public surface of the stationary volume without a GPU: pdwt_volume_create_swt, pdwt_volume_is_swt and pdwt_volume_layout_swt
are declared in include/pypwt_amd.h, exported by both product libraries and bound in pypwt_amd/_lib.py; the layout is a pure host
function that gives the level clamp of tests/volume_swt_ref.py and a block of (3 + 8 L) volumes plus alignment; bad sizes are
refused before any device call; and creating a volume on a machine without a HIP device fails with PDWT_ERR_HIP."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import volume_swt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pdwt_volume_create_swt", "pdwt_volume_is_swt", "pdwt_volume_layout_swt")


@pytest.fixture(scope="module")
def libs():
    from pypwt_amd.build import build_library
    build_library(verbose=False)
    build_library(verbose=False, variant="f64")
    from pypwt_amd import _lib
    return {4: _lib.load(), 8: _lib.load("f64")}


def layout(lib, shape, wname, levels, size):
    nlev, nbytes = C.c_int(-1), C.c_longlong(-1)
    rc = lib.pdwt_volume_layout_swt(shape[0], shape[1], shape[2], wname.encode(), levels, C.byref(nlev), C.byref(nbytes), size)
    return rc, nlev.value, nbytes.value


def test_the_three_functions_are_declared_exported_and_bound(libs):
    from pypwt_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pypwt_amd.h")).read(), flags=re.S)
    bench = open(os.path.join(ROOT, "include", "pypwt_amd_bench.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n not in bench, n  # no new function among the measurement hooks
        assert n in doc, n
        assert n in _lib.SIGNATURES
        for lib in libs.values():
            assert hasattr(lib, n), n
    # the constructor's arguments are pdwt_volume_create's
    args = lambda name: re.search(r"\b%s\s*\((.*?)\)" % name, txt, flags=re.S).group(1).split()
    assert args("pdwt_volume_create_swt") == args("pdwt_volume_create")
    assert _lib.SIGNATURES["pdwt_volume_create_swt"] == _lib.SIGNATURES["pdwt_volume_create"]


def test_python_class_takes_do_swt():
    from pypwt_amd import Wavelets3D, Wavelets3D64
    for cls in (Wavelets3D, Wavelets3D64):
        p = inspect.signature(cls.__init__).parameters
        assert list(p) == ["self", "vol", "wname", "levels", "device", "stream", "do_swt"] and p["do_swt"].default == 0
    assert "swtn" in Wavelets3D.__doc__ and "aaa" in Wavelets3D.__doc__


@pytest.mark.parametrize("shape,wname,asked", [((8, 8, 8), "haar", 3), ((12, 16, 20), "haar", 3), ((5, 7, 9), "haar", 2), ((9, 10, 13), "db2", 1),
                                               ((24, 24, 28), "db2", 3), ((56, 56, 60), "db4", 3), ((4, 40, 44), "db20", 1),
                                               ((256, 256, 256), "db4", 3), ((64, 64, 64), "db4", 9), ((33, 31, 35), "sym8", 0)])
def test_layout_clamp_and_footprint(libs, shape, wname, asked):
    L = volume_swt_ref.clamp_levels(shape, volume_swt_ref.hlen_of(wname), asked)
    n = int(np.prod(shape))
    for size, lib in libs.items():
        for ask in (size, 0):  # 0: the library's own pdwt_real
            rc, nlev, nbytes = layout(lib, shape, wname, asked, ask)
            assert rc == 1 + 7 * L and nlev == L, (shape, wname, asked, rc, nlev)
            volumes = (3 + 8 * L) * n * size
            # every one of the 2 + 4 L buffers is rounded up to 256 B; behind them the operators' sums (16 doubles per level, two per
            # piece of the sweeps -- at most 8 * 128 + 8 pieces per level --, 8 thresholds per level) and 256 B of slack
            extra = (2 + 4 * L) * 255 + (L * 16 * 8 + 255) + (L * 2 * (8 * 128 + 8) * 8 + 255) + (L * 8 * size + 255) + 256
            assert volumes + 16 <= nbytes <= volumes + extra, (shape, wname, size, nbytes - volumes, extra)
            assert nbytes % 256 == 0
        # either library answers for the other's type
        assert layout(lib, shape, wname, asked, 4)[2] == layout(libs[4], shape, wname, asked, 0)[2]
        assert layout(lib, shape, wname, asked, 8)[2] == layout(libs[8], shape, wname, asked, 0)[2]


def test_python_layout_helper(libs):
    from pypwt_amd.volume import volume_layout_swt
    assert volume_layout_swt((56, 56, 60), "db4", 3) == layout(libs[4], (56, 56, 60), "db4", 3, 4)[1:]
    assert volume_layout_swt((56, 56, 60), "db4", 3, np.float64) == layout(libs[8], (56, 56, 60), "db4", 3, 8)[1:]


def test_layout_refuses_what_create_refuses(libs):
    from pypwt_amd import _lib
    from oracle import oracle
    odd = [w for w in oracle.filter_table()["order"] if oracle.filters(w)[0] & 1]
    for lib in libs.values():
        for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-3, 8, 8)):
            assert layout(lib, shape, "db2", 1, 0)[0] == _lib.ERR_ARG, shape
        assert layout(lib, (32768, 8, 8), "haar", 1, 0)[0] == _lib.ERR_ARG
        assert b"32767" in lib.pdwt_last_error()
        assert layout(lib, (32767, 8, 8), "haar", 1, 0)[0] == 8
        assert layout(lib, (8, 8, 8), "nope", 1, 0)[0] == _lib.ERR_WAVELET
        assert layout(lib, (8, 8, 8), "db2", 1, 3)[0] == _lib.ERR_ARG  # sizeof_real
        for w in odd:
            assert layout(lib, (16, 16, 16), w, 1, 0)[0] == _lib.ERR_UNSUPPORTED, w
        assert lib.pdwt_volume_layout_swt(8, 8, 8, b"db2", 1, None, None, 0) == 8  # both outputs are optional
        assert lib.pdwt_volume_is_swt(None) == _lib.ERR_ARG
        # the same refusals from the constructor, before any device call
        h = _lib.handle_t()
        assert lib.pdwt_volume_create_swt(None, 1, 8, 8, b"db2", 1, 1, -1, None, C.byref(h)) == _lib.ERR_ARG
        assert lib.pdwt_volume_create_swt(None, 32768, 8, 8, b"haar", 1, 1, -1, None, C.byref(h)) == _lib.ERR_ARG
        assert lib.pdwt_volume_create_swt(None, 8, 8, 8, b"nope", 1, 1, -1, None, C.byref(h)) == _lib.ERR_WAVELET
        assert lib.pdwt_volume_create_swt(None, 8, 8, 8, b"db2", 1, 1, -1, None, None) == _lib.ERR_ARG
        assert not h


def test_without_a_device_create_swt_fails_with_err_hip(libs):
    """No CPU path: on a machine without a HIP device the constructor returns PDWT_ERR_HIP and the Python class raises."""
    import subprocess
    import sys
    if libs[4].pdwt_device_count() > 0:
        pytest.skip("a HIP device is present")
    from pypwt_amd import _lib
    h = _lib.handle_t()
    for lib in libs.values():
        assert lib.pdwt_volume_create_swt(None, 8, 8, 8, b"db2", 1, 1, -1, None, C.byref(h)) == _lib.ERR_HIP
        assert b"no HIP device" in lib.pdwt_last_error() and not h
    code = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
            "from pypwt_amd import Wavelets3D\n"
            "try:\n"
            "    Wavelets3D(np.zeros((8, 8, 8), np.float32), 'db2', 1, do_swt=1); print('CREATED')\n"
            "except Exception as e: print('RAISED', type(e).__name__)\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env).stdout
    assert "RAISED PdwtError" in out, out
