"""The stationary 3D transform of volumes on the GPU (`Wavelets3D(..., do_swt=1)`, `Wavelets3D64`; pdwt_volume_create_swt) against
the per-axis composition of tests/volume_swt_ref.py, which tests/test_volume_swt_ref_cpu.py pins to pywt.swtn / pywt.iswtn and to
the oracle's 2D SWT.

Bounds, fp32 -- those of tests/test_gpu_volume.py with the fp32 composition as `ref32`:
  * a band / an inverse against the fp64 composition: 1.5e-6 * (1 + levels) * max(max|ref|, 1), or twice the error of the fp32
    composition itself against the fp64 one if that is more (`tol32`);
  * round trip: 7e-4 * scale / 255, or twice the fp32 composition's own round-trip error if that is more;
  * thresholds: bit for bit volume_swt_ref.threshold applied to the bands read before;
  * norms: n * 2^-53 relative to numpy's float64 sums over the returned bands (tighter than an rtol of 1e-5).
fp64: 1e-12 * max|ref| per band.
"""
import ctypes as C

import numpy as np
import pytest

import ops_ref
import volume_swt_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu

SCALE = 255.0
# (shape, wavelet, levels asked for)
CASES = [((8, 8, 8), "haar", 3),        # dilation 4 on the smallest cube
         ((12, 16, 20), "haar", 3),     # Nz not a power of two, f = 4, orbits of 3
         ((5, 7, 9), "haar", 2),        # all odd, P = 63, dword path, gcd(2, 5) = 1: one orbit
         ((9, 10, 13), "db2", 1),       # P % 4 = 2
         ((24, 24, 28), "db2", 3),
         ((56, 56, 60), "db4", 3),
         ((4, 40, 44), "db20", 1),      # depth far below the filter
         ((6, 101, 331), "db2", 1),     # many column groups plus a remainder
         ((40, 12, 12), "db9", 1)]      # the LDS-taps path
IDS = ["%dx%dx%d-%s-L%d" % (s + (w, l)) for s, w, l in CASES]


@pytest.fixture(scope="module")
def classes():
    oracle.build()
    from pypwt_amd import Wavelets3D, Wavelets3D64
    return {np.float32: Wavelets3D, np.float64: Wavelets3D64}


_REF = {}


def ref_of(case):
    """Seeded data and the composition's results for one case, computed once and shared (nothing here is modified later):
    x, levels, fwd64 / fwd32 (bands), rt32 (the fp32 composition's round trip), coef (random coefficients), inv64 / inv32."""
    if case in _REF:
        return _REF[case]
    shape, wname, asked = case
    levels = ref.clamp_levels(shape, ref.hlen_of(wname), asked)
    rng = np.random.default_rng(1000 * sum(shape) + asked)
    x = rng.uniform(0.0, SCALE, shape).astype(np.float32)
    r = {"x": x, "levels": levels}
    r["fwd64"] = ref.forward(x, wname, levels, "full")
    r["fwd32"] = ref.forward(x, wname, levels, False)
    r["rt32"] = ref.inverse(r["fwd32"], wname, levels, False)
    r["coef"] = [(rng.standard_normal(shape) * 50.0).astype(np.float32) for _ in range(1 + 7 * levels)]
    r["inv64"] = ref.inverse([c.astype(np.float64) for c in r["coef"]], wname, levels, "full")
    r["inv32"] = ref.inverse(r["coef"], wname, levels, False)
    for v in r.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _REF[case] = r
    return r


def tol32(ref64, ref32, levels):
    rule = 1.5e-6 * (1 + levels) * max(float(np.abs(ref64).max()), 1.0)
    own = 2.0 * float(np.abs(ref32.astype(np.float64) - ref64).max())
    return max(rule, own)


def close32(got, ref64, ref32, levels, what):
    assert got.dtype == np.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    tol = tol32(ref64, ref32, levels)
    print(what, "err %.3g tol %.3g" % (err, tol))
    assert err <= tol, (what, err, tol)


def close64(got, ref64, what):
    assert got.dtype == np.float64 and got.shape == ref64.shape, (what, got.dtype, got.shape)
    err, tol = float(np.abs(got - ref64).max()), 1e-12 * float(np.abs(ref64).max())
    print(what, "err %.3g tol %.3g" % (err, tol))
    assert err <= tol, (what, err, tol)


def all_bands(W):
    return [W.coeff_only(num) for num in range(W.nbands)]


# ---------------------------------------------------------------------------------------------------------------- fp32

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_equals_the_composition(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked, do_swt=1)
    assert W.levels == r["levels"] and W.shape == shape and W.nbands == 1 + 7 * r["levels"]
    assert W.do_swt == 1 and W.info()["do_swt"] == 1 and "swt" in repr(W)
    assert [W.band_shape(n) for n in range(W.nbands)] == ref.band_shapes(shape, r["levels"])
    for num in range(W.nbands):
        d, rr, cc = C.c_int(), C.c_int(), C.c_int()
        assert W._lib.pdwt_volume_coeff_count(W._h, num, C.byref(d), C.byref(rr), C.byref(cc)) == int(np.prod(shape))
        assert (d.value, rr.value, cc.value) == shape
    W.forward()
    for num, g in enumerate(all_bands(W)):
        close32(g, r["fwd64"][num], r["fwd32"][num], r["levels"], (case, "band", num))
    co = W.coeffs
    assert len(co) == r["levels"] + 1 and all(sorted(d) == list(ref.KEYS) for d in co[1:])
    assert np.array_equal(co[1]["ddd"], W.coeff_only(ref.num_of(1, "ddd")))
    assert np.array_equal(W.image, r["x"])  # the forward leaves the image alone


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inverse_alone_from_set_coeff(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](np.zeros(shape, dtype=np.float32), wname, asked, do_swt=1)
    for num, c in enumerate(r["coef"]):
        W.set_coeff(c, num)
    for num, c in enumerate(r["coef"]):  # after ALL were set: a half-band view that overlapped its neighbour would show here
        assert np.array_equal(W.coeff_only(num), c), (case, num)
    W.inverse()
    close32(W.image, r["inv64"], r["inv32"], r["levels"], (case, "inverse"))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_round_trip(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked, do_swt=1)
    W.forward()
    W.inverse()
    err = float(np.abs(W.image.astype(np.float64) - r["x"]).max())
    own = float(np.abs(r["rt32"].astype(np.float64) - r["x"]).max())
    tol = max(7e-4 * SCALE / 255.0, 2.0 * own)
    print(case, "round trip err %.3g tol %.3g (fp32 composition %.3g)" % (err, tol, own))
    assert err <= tol, (case, err, tol)


# ---------------------------------------------------------------------------------------------------------------- fp64

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_forward_inverse_round_trip(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    L = r["levels"]
    x = r["x"].astype(np.float64)
    W = classes[np.float64](x, wname, asked, do_swt=1)
    assert W.levels == L
    W.forward()
    for num, g in enumerate(all_bands(W)):
        close64(g, r["fwd64"][num], (case, "band", num))
    W.inverse()
    close64(W.image, x, (case, "round trip"))
    coef = [c.astype(np.float64) for c in r["coef"]]
    for num, c in enumerate(coef):
        W.set_coeff(c, num)
    for num, c in enumerate(coef):
        assert np.array_equal(W.coeff_only(num), c)
    W.inverse()
    close64(W.image, r["inv64"], (case, "inverse"))


def test_fp64_thresholds_and_norms(classes):
    case = CASES[4]
    shape, wname, asked = case
    r = ref_of(case)
    L = r["levels"]
    W = classes[np.float64](r["x"].astype(np.float64), wname, asked, do_swt=1)
    W.forward()
    before = all_bands(W)
    n = sum(b.size for b in before)
    n1, n2 = float(sum(np.abs(b).sum() for b in before)), float(sum((b * b).sum() for b in before))
    g1, g2 = W.norms()
    assert abs(g1 - n1) <= n * 2.0 ** -53 * n1 and abs(g2 - n2) <= (n + 2) * 2.0 ** -53 * n2, (g1, n1, g2, n2)
    W.soft_threshold(17.25, 1, 1)
    for num, (g, w) in enumerate(zip(all_bands(W), ref.threshold(before, L, "soft", 17.25, 1, 1))):
        assert ops_ref.same_bits(g, w), (case, num)


# ------------------------------------------------------------------------------------------------- every instantiation
DB = ["db%d" % k for k in range(1, 21)]
DB_SHAPE = (40, 8, 12)


@pytest.mark.parametrize("wname", DB)
def test_every_filter_length_runs_on_the_device_in_both_directions(classes, wname):
    """db1 .. db20: 2 .. 40 taps, every even length the depth kernels are instantiated for; planes of 96 samples take the wide
    access of each, and the depth of 40 is below the longer filters' dilated support only at 40 taps."""
    case = (DB_SHAPE, wname, 1)
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, 1, do_swt=1)
    assert (W.levels, W.hlen) == (1, 2 * int(wname[2:]))
    assert W.depth_schedule(1)[0] == (4 if W.hlen <= 16 else 2)
    W.forward()
    for num, g in enumerate(all_bands(W)):
        close32(g, r["fwd64"][num], r["fwd32"][num], 1, (case, "band", num))
    for num, c in enumerate(r["coef"]):
        W.set_coeff(c, num)
    W.inverse()
    close32(W.image, r["inv64"], r["inv32"], 1, (case, "inverse"))


# -------------------------------------------------------------------------------------------------------- segments
def run_both(W, r):
    """(bands of the forward of r's volume, image of the inverse alone from r's random coefficients)"""
    W.set_image(r["x"])
    W.forward()
    bands = all_bands(W)
    for num, c in enumerate(r["coef"]):
        W.set_coeff(c, num)
    W.inverse()
    return bands, W.image


@pytest.mark.parametrize("case", [CASES[4], CASES[8]], ids=[IDS[4], IDS[8]])
def test_forced_segments_give_the_choosers_bits(classes, case):
    """Segments of 1 and 3 steps and one whole walk per orbit: the same arithmetic per output slice, so the same bits."""
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked, do_swt=1)
    L = r["levels"]
    steps = [shape[0] // np.gcd(1 << (l - 1), shape[0]) for l in range(1, L + 1)]
    chosen = [W.depth_schedule(l) for l in range(1, L + 1)]
    want_bands, want_img = run_both(W, r)
    for num, g in enumerate(want_bands):
        close32(g, r["fwd64"][num], r["fwd32"][num], L, (case, "chooser", num))
    for seg in (1, 3, None):
        for l in range(1, L + 1):
            s = steps[l - 1] if seg is None else min(seg, steps[l - 1])
            W._set_depth_segments(l, s, s)
            assert W.depth_schedule(l) == (chosen[l - 1][0], s, s)
        bands, img = run_both(W, r)
        for num, (g, w) in enumerate(zip(bands, want_bands)):
            assert np.array_equal(g, w), (case, seg, num)
        assert np.array_equal(img, want_img), (case, seg)
    for l in range(1, L + 1):
        W._set_depth_segments(l, 0, 0)  # 0 restores the chooser's value
        assert W.depth_schedule(l) == chosen[l - 1]
    with pytest.raises(Exception):
        W._set_depth_segments(1, steps[0] + 1, 1)


WALK_CASE = ((128, 128, 136), "db4", 3)  # level 1: 17 column groups x 128 steps = 2176 workgroups of one step


def test_the_shipped_chooser_cuts_segments_of_several_steps(classes):
    """(128, 64, 64), four column groups, is 512 one-step workgroups at level 1: one round, so the chooser leaves one step per
    workgroup, and so it does up to 16 column groups.  Planes of 128 x 136 are the first multiple of eight columns with 17: 2176
    one-step workgroups are more than a chip of 256 CUs can keep resident at ANY occupancy (at most 8 workgroups of 256 threads per
    CU, 2048 -- fewer where the kernel's registers allow fewer, and then the segments only get longer), so two steps per segment
    halve the rounds.  Nothing is assumed about the occupancy: the schedule the volume reports is what is asserted.  fp64
    composition only (the rule's first arm, the tighter one)."""
    shape, wname, asked = WALK_CASE
    x = np.random.default_rng(sum(shape)).uniform(0.0, SCALE, shape).astype(np.float32)
    W = classes[np.float32](x, wname, asked, do_swt=1)
    L = W.levels
    assert L == 3
    sched = [W.depth_schedule(l) for l in range(1, L + 1)]
    print("depth schedule", sched)
    assert sched[0][0] == 4 and sched[0][1] >= 2 and sched[0][2] >= 2, sched
    fwd64 = ref.forward(x, wname, L, "full")
    W.forward()
    for num in range(W.nbands):
        g, want = W.coeff_only(num), fwd64[num]
        err, tol = float(np.abs(g.astype(np.float64) - want).max()), 1.5e-6 * (1 + L) * max(float(np.abs(want).max()), 1.0)
        print("band", num, "err %.3g tol %.3g" % (err, tol))
        assert err <= tol, (num, err, tol)
    W.inverse()
    err = float(np.abs(W.image.astype(np.float64) - x).max())
    print("round trip err %.3g" % err)
    assert err <= 7e-4 * SCALE / 255.0, err


# ---------------------------------------------------------------------------------------------------------- thresholds
THR_CASE = CASES[4]  # (24, 24, 28) db2: three levels


@pytest.mark.parametrize("op", ["soft", "hard"])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("do_app", [0, 1])
def test_thresholds_bit_for_bit(classes, op, normalize, do_app):
    shape, wname, asked = THR_CASE
    r = ref_of(THR_CASE)
    L = r["levels"]
    assert L == 3
    W = classes[np.float32](r["x"], wname, asked, do_swt=1)
    W.forward()
    before = all_bands(W)
    beta = 21.5
    getattr(W, op + "_threshold")(beta, do_app, normalize)
    want = ref.threshold(before, L, op, beta, do_app, normalize)
    after = all_bands(W)
    for num, (g, w) in enumerate(zip(after, want)):
        assert ops_ref.same_bits(g, w), (op, normalize, do_app, num)
        if num > 0:
            assert not np.array_equal(g, before[num]), (num, "beta bites in every detail band")
    assert np.array_equal(after[0], before[0]) == (not (do_app and op == "soft"))  # (hard: every |A_L| is far above beta)
    # the intermediates A_1 .. A_{L-1} are no coefficients: a sweep that touched them would show in nothing but the inverse
    W.inverse()
    inv64 = ref.inverse([b.astype(np.float64) for b in want], wname, L, "full")
    inv32 = ref.inverse(want, wname, L, False)
    close32(W.image, inv64, inv32, L, (op, normalize, do_app, "inverse after threshold"))


@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[7]], ids=[IDS[2], IDS[4], IDS[7]])
def test_norms(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked, do_swt=1)
    W.forward()
    bands = all_bands(W)
    n = sum(b.size for b in bands)
    n1 = float(sum(np.abs(b.astype(np.float64)).sum() for b in bands))
    n2 = float(sum((b.astype(np.float64) ** 2).sum() for b in bands))
    g1, g2 = W.norm1(), W.norm2sq()
    assert (g1, g2) == W.norms()
    assert abs(g1 - n1) <= n * 2.0 ** -53 * n1, (g1, n1)
    assert abs(g2 - n2) <= n * 2.0 ** -53 * n2, (g2, n2)


# --------------------------------------------------------------------------------------------------------------- state

def test_state_machine(classes):
    from pypwt_amd import _lib
    case = CASES[4]
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked, do_swt=1)
    lib = W._lib
    assert lib.pdwt_volume_is_swt(W._h) == 1
    assert W.info()["state"] == _lib.STATE_INIT
    W.forward()
    assert W.info()["state"] == _lib.STATE_FORWARD
    W.soft_threshold(10.0)
    W.inverse()
    assert W.info()["state"] == _lib.STATE_INVERSE
    img = W.image
    # a second inverse in a row: refused, nothing done
    assert lib.pdwt_volume_inverse(W._h) == _lib.ERR_STATE
    assert np.array_equal(W.image, img) and W.info()["state"] == _lib.STATE_INVERSE
    # coefficient getters, thresholds and norms are refused after the inverse
    buf = np.zeros(W.band_shape(0), dtype=np.float32)
    assert lib.pdwt_volume_get_coeff(W._h, buf.ctypes.data_as(C.c_void_p), 0) == 0
    with pytest.raises(RuntimeError):
        W.coeff_only(3)
    assert lib.pdwt_volume_soft_threshold(W._h, 1.0, 0, 0) == _lib.ERR_STATE
    out = (C.c_double * 2)()
    assert lib.pdwt_volume_norms(W._h, out) == _lib.ERR_STATE
    assert lib.pdwt_volume_get_coeff(W._h, buf.ctypes.data_as(C.c_void_p), 99) == _lib.ERR_ARG
    # a new volume on the same object: nothing stale is left in the intermediates
    other = r["x"][::-1, ::-1, ::-1].copy()
    W.set_image(other)
    assert W.info()["state"] == _lib.STATE_INIT
    W.forward()
    L = r["levels"]
    ref64 = ref.forward(other, wname, L, "full")
    ref32 = ref.forward(other, wname, L, False)
    for num, g in enumerate(all_bands(W)):
        close32(g, ref64[num], ref32[num], L, ("second volume", num))
    # set_coeff of the approximation after an inverse makes the coefficients current again
    W.inverse()
    W.set_coeff(W.coeff_device(0), 0)  # its own buffer: nothing is copied
    assert W.info()["state"] == _lib.STATE_FORWARD
    W.hard_threshold(5.0)
    W.inverse()
    W.synchronize()
    assert W._stream()


def test_the_operators_that_are_out_of_scope_raise(classes):
    from pypwt_amd import _lib
    case = CASES[3]
    r = ref_of(case)
    W = classes[np.float32](r["x"], case[1], case[2], do_swt=1)
    W.forward()
    calls = {"band_stats": lambda: W.band_stats(), "estimate_sigma": lambda: W.estimate_sigma(),
             "threshold_bands": lambda: W.threshold_bands(np.ones(W.nbands, dtype=np.float32)), "denoise": lambda: W.denoise(),
             "select_magnitude": lambda: W.select_magnitude(k=3), "keep_largest": lambda: W.keep_largest(fraction=0.5),
             "norms_device": lambda: W.norms_device(), "last_thresholds": lambda: W.last_thresholds(),
             "last_sparsify": lambda: W.last_sparsify(), "read_norms": lambda: W.read_norms()}
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match=name):
            call()
    # the C entry points themselves: PDWT_ERR_UNSUPPORTED with a message naming the call, nothing allocated
    lib = W._lib
    p = C.c_void_p()
    for name, args in (("pdwt_volume_norms_async", (None,)), ("pdwt_volume_adaptive_slots", (C.byref(p), None, None)),
                       ("pdwt_volume_sparsify_slots", (C.byref(p), None)), ("pdwt_volume_band_stats_async", (None,)),
                       ("pdwt_volume_estimate_sigma_async", (1, None)), ("pdwt_volume_denoise_async", (0, 0, None, 1)),
                       ("pdwt_volume_select_magnitude_async", (5, 0, None, None)), ("pdwt_volume_keep_largest_async", (5, 0)),
                       ("pdwt_volume_threshold_bands", (0, C.byref(p), 0))):
        assert getattr(lib, name)(W._h, *args) == _lib.ERR_UNSUPPORTED, name
        assert name.encode() in lib.pdwt_last_error(), (name, lib.pdwt_last_error())
    # the coefficients are as the forward left them
    for num, g in enumerate(all_bands(W)):
        close32(g, r["fwd64"][num], r["fwd32"][num], r["levels"], ("after the refusals", num))


TORCH_CODE = r"""
import sys
import torch                                       # first: the library then shares torch's HIP runtime (INTEGRATION.md)
assert torch.cuda.is_available(), "torch sees no GPU"   # no way round: without a device this process fails, and so does the test
import numpy as np
sys.path.insert(0, "tests")
import volume_swt_ref as ref
from pypwt_amd import Wavelets3D
shape, wname, L = (24, 24, 28), "db2", 3
x = np.random.default_rng(77).uniform(0.0, 255.0, shape).astype(np.float32)
f64, f32 = ref.forward(x, wname, L, "full"), ref.forward(x, wname, L, False)
t = torch.from_numpy(x.copy()).to("cuda")
W = Wavelets3D(t, wname, L, do_swt=1)
assert np.array_equal(W.image, x)
W.forward()
W.synchronize()
for num in range(W.nbands):
    view = torch.as_tensor(W.coeff_device(num), device="cuda")        # device view out: zero copy
    assert tuple(view.shape) == shape and view.data_ptr() == W._lib.pdwt_volume_coeff_ptr(W._h, num)
    g = view.cpu().numpy()
    assert np.array_equal(g, W.coeff_only(num))
    tol = max(1.5e-6 * (1 + L) * max(float(np.abs(f64[num]).max()), 1.0), 2.0 * float(np.abs(f32[num].astype(np.float64) - f64[num]).max()))
    assert float(np.abs(g.astype(np.float64) - f64[num]).max()) <= tol, num
t2 = (t * 0.5).contiguous()                                          # a torch expression as the new volume
W.set_image(t2)
torch.cuda.synchronize()
assert np.array_equal(W.image, x * np.float32(0.5))
img = torch.as_tensor(W.image_device, device="cuda")
assert tuple(img.shape) == shape and np.array_equal(img.cpu().numpy(), W.image)
W.forward()
c = torch.full(shape, 3.25, device="cuda")                           # a coefficient from a device tensor
W.set_coeff(c, 5)
assert np.array_equal(W.coeff_only(5), np.full(shape, 3.25, dtype=np.float32))
print("TORCH_OK")
"""


def test_input_from_a_torch_tensor_and_device_views():
    """Torch tensor in, device view out -- in a child process, as tests/test_gpu_ops.py does: torch must be imported before the
    library so that both share torch's HIP runtime, whatever ran in this process before.  The child has no way to
    pass without doing the work: it ends with TORCH_OK or with a non-zero status.  A host without torch shows as a skip, decided here
    before anything runs."""
    import os
    import subprocess
    import sys
    import importlib.util
    if importlib.util.find_spec("torch") is None:  # (looked up, not imported: this process stays as it was)
        pytest.skip("torch is not installed")
    r = subprocess.run([sys.executable, "-c", TORCH_CODE], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-500:])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("TORCH_OK"), r.stdout[-1000:]


def test_a_decimated_and_a_stationary_volume_alive_at_once(classes):
    import volume_ref
    case = CASES[4]
    shape, wname, asked = case
    r = ref_of(case)
    Wd = classes[np.float32](r["x"], wname, asked)
    Ws = classes[np.float32](r["x"], wname, asked, do_swt=1)
    assert Wd._lib.pdwt_volume_is_swt(Wd._h) == 0 and Wd.do_swt == 0 and "swt" not in repr(Wd)
    Ld = Wd.levels
    Ws.forward()
    Wd.forward()
    d64, d32 = volume_ref.forward(r["x"], wname, Ld, "full"), volume_ref.forward(r["x"], wname, Ld, False)
    for num, g in enumerate(all_bands(Wd)):
        close32(g, d64[num], d32[num], Ld, ("decimated beside stationary", num))
    for num, g in enumerate(all_bands(Ws)):
        close32(g, r["fwd64"][num], r["fwd32"][num], r["levels"], ("stationary beside decimated", num))
    Wd.inverse()
    Ws.inverse()
    assert float(np.abs(Wd.image.astype(np.float64) - r["x"]).max()) <= 7e-4
    assert float(np.abs(Ws.image.astype(np.float64) - r["x"]).max()) <= max(7e-4, 2.0 * float(np.abs(r["rt32"].astype(np.float64) - r["x"]).max()))
