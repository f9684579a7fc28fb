"""Which pdwt_volume_* call is refused, with which code and which pdwt_last_error text: one fixed list of calls on a decimated and
on a stationary volume, fp32 and fp64, compared for equality with tests/golden/volume_refusals.json.

The fixture is a recording of this same list, made once on the GPU by the commit BEFORE the volume handle was split into
pdwt::VolumeDwt and pdwt::VolumeSwt (`python tests/test_gpu_volume_refusals.py --record`), never by the code under test.  The
messages do not depend on the precision, so one walk per (volume, mode) is stored; the recording refuses to write anything else.
The walk opens with a call that fails, so the message it reads first is its own.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "volume_refusals.json")
VOLUMES = [((8, 6, 10), "haar"), ((9, 8, 8), "db2")]
LEVELS = 2
VARIANTS = {"f32": (np.float32, C.c_float), "f64": (np.float64, C.c_double)}


def key_of(shape, wname, do_swt):
    return "%dx%dx%d-%s-%s" % (shape + (wname, "swt" if do_swt else "dwt"))


def walk(variant, shape, wname, do_swt):
    """[label, value, message] of every call of the list, in order; value is the return code (or [code, state])."""
    from pypwt_amd import _lib
    lib = _lib.load(variant)
    dtype, real = VARIANTS[variant]
    realp = C.POINTER(real)
    out = []

    def rec(label, value):
        out.append([label, value, _lib.last_error(lib)])

    rng = np.random.default_rng(7)
    x = rng.uniform(0.0, 255.0, shape).astype(dtype)
    buf = np.zeros(int(np.prod(shape)), dtype)  # at least as large as any band of either transform
    p = buf.ctypes.data
    two = (C.c_double * 2)()
    taps = (real * 64)()
    fp = C.cast(taps, realp)
    N = None

    def state(h):
        st = C.c_int(-1)
        rc = lib.pdwt_volume_get_info(h, None, None, None, None, None, C.byref(st))
        return [rc, st.value]

    # ---- every entry point with a null handle (forward first: it fails, so every message below belongs to this walk)
    rec("null forward", lib.pdwt_volume_forward(N))
    rec("null inverse", lib.pdwt_volume_inverse(N))
    rec("null get_info", lib.pdwt_volume_get_info(N, None, None, None, None, None, None))
    rec("null get_image", lib.pdwt_volume_get_image(N, p))
    rec("null set_image", lib.pdwt_volume_set_image(N, p, 0))
    rec("null coeff_count", lib.pdwt_volume_coeff_count(N, 0, None, None, None))
    rec("null get_coeff", lib.pdwt_volume_get_coeff(N, p, 0))
    rec("null set_coeff", lib.pdwt_volume_set_coeff(N, p, 0, 0))
    rec("null image_ptr", lib.pdwt_volume_image_ptr(N))
    rec("null coeff_ptr", lib.pdwt_volume_coeff_ptr(N, 0))
    rec("null soft_threshold", lib.pdwt_volume_soft_threshold(N, 1.0, 0, 0))
    rec("null hard_threshold", lib.pdwt_volume_hard_threshold(N, 1.0, 0, 0))
    rec("null norms", lib.pdwt_volume_norms(N, two))
    rec("null band_stats_async", lib.pdwt_volume_band_stats_async(N, None))
    rec("null norms_async", lib.pdwt_volume_norms_async(N, None))
    rec("null estimate_sigma_async", lib.pdwt_volume_estimate_sigma_async(N, 1, None))
    rec("null threshold_bands", lib.pdwt_volume_threshold_bands(N, 0, p, 0))
    rec("null denoise_async", lib.pdwt_volume_denoise_async(N, 0, 0, None, 1))
    rec("null adaptive_slots", lib.pdwt_volume_adaptive_slots(N, None, None, None))
    rec("null select_magnitude_async", lib.pdwt_volume_select_magnitude_async(N, 1, 0, None, None))
    rec("null keep_largest_async", lib.pdwt_volume_keep_largest_async(N, 1, 0))
    rec("null sparsify_slots", lib.pdwt_volume_sparsify_slots(N, None, None))
    rec("null read", lib.pdwt_volume_read(N, p, p, 4))
    rec("null synchronize", lib.pdwt_volume_synchronize(N))
    rec("null stream", lib.pdwt_volume_stream(N) or 0)
    rec("null depth_schedule", lib.pdwt_volume_depth_schedule(N, 1, None, None, None))
    rec("null set_filters", lib.pdwt_volume_set_filters(N, 2, fp, fp, fp, fp))
    rec("null set_depth_segments", lib.pdwt_volume_set_depth_segments(N, 1, 0, 0))
    rec("null is_swt", lib.pdwt_volume_is_swt(N))
    rec("null destroy", lib.pdwt_volume_destroy(N))
    create = lib.pdwt_volume_create_swt if do_swt else lib.pdwt_volume_create
    rec("create out=null", create(x.ctypes.data, shape[0], shape[1], shape[2], wname.encode(), LEVELS, 1, -1, None, None))

    h = C.c_void_p()
    rc = create(x.ctypes.data, shape[0], shape[1], shape[2], wname.encode(), LEVELS, 1, -1, None, C.byref(h))
    rec("create", rc)
    assert rc == 0 and h.value, _lib.last_error(lib)
    try:
        L, hlen = C.c_int(), C.c_int()
        assert lib.pdwt_volume_get_info(h, None, None, None, C.byref(L), C.byref(hlen), None) == 0
        L, hlen, nb = L.value, hlen.value, 1 + 7 * L.value
        rec("levels hlen", [L, hlen])
        rec("is_swt", lib.pdwt_volume_is_swt(h))
        rec("forward", lib.pdwt_volume_forward(h))
        rec("state", state(h))

        # ---- null data arguments
        rec("get_image dst=null", lib.pdwt_volume_get_image(h, None))
        rec("set_image src=null", lib.pdwt_volume_set_image(h, None, 0))
        rec("get_coeff dst=null", lib.pdwt_volume_get_coeff(h, None, 0))
        rec("set_coeff src=null", lib.pdwt_volume_set_coeff(h, None, 0, 0))
        rec("norms out=null", lib.pdwt_volume_norms(h, None))
        rec("read dst=null", lib.pdwt_volume_read(h, None, p, 4))
        rec("read bytes<0", lib.pdwt_volume_read(h, p, p, -1))

        # ---- num and level out of range
        for num in (-1, nb):
            rec("coeff_count num=%d" % num, lib.pdwt_volume_coeff_count(h, num, None, None, None))
            rec("get_coeff num=%d" % num, lib.pdwt_volume_get_coeff(h, p, num))
            rec("set_coeff num=%d" % num, lib.pdwt_volume_set_coeff(h, p, num, 0))
            rec("coeff_ptr num=%d" % num, lib.pdwt_volume_coeff_ptr(h, num))
        for level in (0, L + 1):
            rec("depth_schedule level=%d" % level, lib.pdwt_volume_depth_schedule(h, level, None, None, None))
            rec("set_depth_segments level=%d" % level, lib.pdwt_volume_set_depth_segments(h, level, 0, 0))

        # ---- the test hooks
        rec("set_filters hlen+2", lib.pdwt_volume_set_filters(h, hlen + 2, fp, fp, fp, fp))
        rec("set_filters null filter", lib.pdwt_volume_set_filters(h, hlen, fp, None, fp, fp))
        rec("set_depth_segments fwd beyond", lib.pdwt_volume_set_depth_segments(h, 1, 1000000, 0))
        rec("set_depth_segments inv beyond", lib.pdwt_volume_set_depth_segments(h, 1, 0, 1000000))
        rec("set_depth_segments negative", lib.pdwt_volume_set_depth_segments(h, L, -1, 0))
        rec("set_depth_segments restore", lib.pdwt_volume_set_depth_segments(h, 1, 0, 0))

        # ---- the operator entry points: bad arguments, then good ones (a stationary volume refuses them all)
        table = np.zeros(nb, dtype)
        tp = table.ctypes.data
        sigma = C.c_double(1.0)
        rec("threshold_bands table=null", lib.pdwt_volume_threshold_bands(h, 0, None, 0))
        rec("threshold_bands op=2", lib.pdwt_volume_threshold_bands(h, 2, tp, 0))
        rec("denoise method=7", lib.pdwt_volume_denoise_async(h, 7, 0, None, 1))
        rec("denoise op=5", lib.pdwt_volume_denoise_async(h, 0, 5, None, 1))
        rec("select_magnitude K=-1", lib.pdwt_volume_select_magnitude_async(h, -1, 0, None, None))
        rec("keep_largest K=-1", lib.pdwt_volume_keep_largest_async(h, -1, 1))

        def operators(tag):
            rec(tag + "band_stats_async", lib.pdwt_volume_band_stats_async(h, None))
            rec(tag + "norms_async", lib.pdwt_volume_norms_async(h, None))
            rec(tag + "estimate_sigma_async", lib.pdwt_volume_estimate_sigma_async(h, 1, None))
            rec(tag + "threshold_bands", lib.pdwt_volume_threshold_bands(h, 0, tp, 0))
            rec(tag + "denoise_async", lib.pdwt_volume_denoise_async(h, 0, 0, C.byref(sigma), 1))
            rec(tag + "adaptive_slots", lib.pdwt_volume_adaptive_slots(h, None, None, None))
            rec(tag + "select_magnitude_async", lib.pdwt_volume_select_magnitude_async(h, 3, 0, None, None))
            rec(tag + "keep_largest_async", lib.pdwt_volume_keep_largest_async(h, 3, 0))
            rec(tag + "sparsify_slots", lib.pdwt_volume_sparsify_slots(h, None, None))

        operators("")
        rec("soft_threshold", lib.pdwt_volume_soft_threshold(h, 1.0, 1, 1))
        rec("hard_threshold", lib.pdwt_volume_hard_threshold(h, 1.0, 0, 0))
        rec("norms", lib.pdwt_volume_norms(h, two))
        rec("state before inverse", state(h))

        # ---- after inverse()
        rec("inverse", lib.pdwt_volume_inverse(h))
        rec("state after inverse", state(h))
        rec("after inverse: inverse", lib.pdwt_volume_inverse(h))
        rec("after inverse: get_coeff", lib.pdwt_volume_get_coeff(h, p, 1))
        rec("after inverse: soft_threshold", lib.pdwt_volume_soft_threshold(h, 1.0, 0, 0))
        rec("after inverse: hard_threshold", lib.pdwt_volume_hard_threshold(h, 1.0, 0, 0))
        rec("after inverse: norms", lib.pdwt_volume_norms(h, two))
        operators("after inverse: ")
        rec("after inverse: coeff_count", lib.pdwt_volume_coeff_count(h, 0, None, None, None))
        rec("after inverse: set_coeff num=1", lib.pdwt_volume_set_coeff(h, p, 1, 0))
        rec("state after set_coeff num=1", state(h))
        rec("after inverse: set_coeff num=0", lib.pdwt_volume_set_coeff(h, p, 0, 0))
        rec("state after set_coeff num=0", state(h))
        rec("restored: norms", lib.pdwt_volume_norms(h, two))
        rec("restored: get_coeff", lib.pdwt_volume_get_coeff(h, p, 1))
        rec("restored: inverse", lib.pdwt_volume_inverse(h))
        rec("set_image", lib.pdwt_volume_set_image(h, x.ctypes.data, 0))
        rec("state after set_image", state(h))
        rec("synchronize", lib.pdwt_volume_synchronize(h))
    finally:
        rec("destroy", lib.pdwt_volume_destroy(h))
    return out


@pytest.fixture(scope="module")
def expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("do_swt", [0, 1], ids=["dwt", "swt"])
@pytest.mark.parametrize("shape,wname", VOLUMES, ids=["8x6x10-haar", "9x8x8-db2"])
def test_refusals_are_the_recorded_ones(expected, shape, wname, do_swt, variant):
    got = walk(variant, shape, wname, do_swt)
    want = expected["walks"][key_of(shape, wname, do_swt)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # what the list is there for: the stationary handle refused every operator, the decimated one none
    refused = [g for g in got if "do_swt" in g[2] and g[1] == -7]
    assert (len(refused) > 0) == bool(do_swt)


def record(commit):
    walks = {}
    for shape, wname in VOLUMES:
        for do_swt in (0, 1):
            w32, w64 = (walk(v, shape, wname, do_swt) for v in ("f32", "f64"))
            assert w32 == w64, "the walks of the two precisions differ: %s" % [p for p in zip(w32, w64) if p[0] != p[1]]
            walks[key_of(shape, wname, do_swt)] = w32
    with open(FIXTURE, "w") as f:
        json.dump({"recorded_by": commit, "walks": walks}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d walks of %d calls into %s" % (len(walks), len(next(iter(walks.values()))), FIXTURE))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if len(sys.argv) not in (3, 4) or sys.argv[1] != "--record":
        raise SystemExit("usage: python tests/test_gpu_volume_refusals.py --record COMMIT [FILE]")
    if len(sys.argv) == 4:
        FIXTURE = sys.argv[3]  # another place for the file
    record(sys.argv[2])
