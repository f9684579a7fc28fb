"""3D DWT of volumes on the GPU (`Wavelets3D`, the pdwt_volume_* ABI) against the composition of the CPU oracle
(tests/volume_ref.py; pinned to pywt.wavedecn by tests/test_volume_ref_cpu.py).

Bounds, fp32:
  * a band / an inverse against the fp64 composition: the project's rule for fp32 against the oracle,
    1.5e-6 * (1 + levels) * max(max|ref|, 1) (tests/test_gpu_parity.py:60), or twice the error of the fp32 composition itself
    against the fp64 one on that band if that is more (the idea behind reconstruction_tol);
  * round trip: 7e-4 * scale / 255, or twice the fp32 composition's own round-trip error if that is more;
  * thresholds: bit for bit tests/ops_ref.py applied to the bands read before;
  * norms: n * 2^-53 relative to numpy's float64 sums over the returned bands (a reordered fp64 sum of n terms).
fp64: 1e-12 * max(max|ref|, 1) per band.

(300, 12, 12) db4 is asked for two levels; the reference's clamp, ilog2(12 / 7) = 0 -> one level, leaves one, and the test follows
the plan's clamp (which it checks against the rule) like every other test of clamped plans.
"""
import ctypes as C

import numpy as np
import pytest

import ops_ref
import volume_ref
from oracle import oracle

pytestmark = pytest.mark.gpu

SCALE = 255.0
# (shape, wavelet, levels asked for)
CASES = [((16, 16, 16), "haar", 2),     # smallest even case
         ((9, 10, 13), "db2", 1),       # all odd-ish sizes, P % 4 = 2
         ((5, 64, 64), "haar", 2),      # odd depth twice: 5 -> 3 -> 2
         ((64, 48, 40), "db2", 3),      # level-3 planes 6 x 5, P odd
         ((24, 20, 28), "db4", 1),      # short-filter path
         ((33, 31, 35), "sym8", 1),     # odd sizes on all axes
         ((40, 40, 44), "db20", 1),     # 40 taps through the strip kernels and the long depth path
         ((6, 101, 331), "db2", 1),     # P odd, many workgroups plus a remainder
         ((300, 12, 12), "db4", 2),     # many depth segments, tiny planes
         ((130, 8, 8), "haar", 3)]      # deep in depth
CASES64 = [CASES[1], CASES[3], CASES[6]]
IDS = ["%dx%dx%d-%s-L%d" % (s + (w, l)) for s, w, l in CASES]
IDS64 = ["%dx%dx%d-%s-L%d" % (s + (w, l)) for s, w, l in CASES64]


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
    levels = volume_ref.clamp_levels(shape, volume_ref.hlen_of(wname), asked)
    rng = np.random.default_rng(1000 * sum(shape) + asked)
    x = rng.uniform(0.0, SCALE, shape).astype(np.float32)
    r = {"x": x, "levels": levels}
    r["fwd64"] = volume_ref.forward(x, wname, levels, "full")
    r["fwd32"] = volume_ref.forward(x, wname, levels, False)
    r["rt32"] = volume_ref.inverse(r["fwd32"], shape, wname, levels, False)
    r["coef"] = [(rng.standard_normal(s) * 50.0).astype(np.float32) for s in volume_ref.band_shapes(shape, levels)]
    r["inv64"] = volume_ref.inverse([c.astype(np.float64) for c in r["coef"]], shape, wname, levels, "full")
    r["inv32"] = volume_ref.inverse(r["coef"], shape, wname, levels, False)
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


def all_bands(W):
    return [W.coeff_only(num) for num in range(W.nbands)]


# ---------------------------------------------------------------------------------------------------------------- fp32

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_equals_the_composition(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked)
    assert W.levels == r["levels"] and W.shape == shape and W.nbands == 1 + 7 * r["levels"]
    assert [W.band_shape(n) for n in range(W.nbands)] == volume_ref.band_shapes(shape, r["levels"])
    W.forward()
    for num, g in enumerate(all_bands(W)):
        close32(g, r["fwd64"][num], r["fwd32"][num], r["levels"], (case, "band", num))
    co = W.coeffs
    assert len(co) == r["levels"] + 1 and all(sorted(d) == list(volume_ref.KEYS) for d in co[1:])
    assert np.array_equal(co[1]["ddd"], W.coeff_only(volume_ref.num_of(1, "ddd")))
    assert np.array_equal(W.image, r["x"])  # the forward leaves the image alone


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inverse_alone_from_set_coeff(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](np.zeros(shape, dtype=np.float32), wname, asked)
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
    W = classes[np.float32](r["x"], wname, asked)
    W.forward()
    W.inverse()
    err = float(np.abs(W.image.astype(np.float64) - r["x"]).max())
    own = float(np.abs(r["rt32"].astype(np.float64) - r["x"]).max())
    tol = max(7e-4 * SCALE / 255.0, 2.0 * own)
    print(case, "round trip err %.3g tol %.3g (fp32 composition %.3g)" % (err, tol, own))
    assert err <= tol, (case, err, tol)


# ------------------------------------------------------------------------------------------------- walks of several steps
# The shapes above are small: the segment chooser gives every workgroup ONE step there (column groups x steps stay below the
# workgroups the chip keeps resident).  These are the smallest shapes at which the shipped chooser cuts segments of two or more
# steps, one per access width -- 16 B, the 8-B path of the long filters, a dword --, so that the register window's shift, the loads
# one step ahead and the wrapping source counter across steps run on the device and are compared with the composition.  They
# are large for the oracle, so only the fp64 composition is computed (once, shared) and the bounds are the rule's first arm
# alone, which is the tighter one: 1.5e-6 * (1 + levels) * max(max|ref|, 1), and 7e-4 * scale / 255 for the round trip.
WALK_CASES = [((256, 160, 128), "db4", 4),   # 20 column groups x 128 steps > 2048 resident workgroups
              ((520, 64, 80), "db9", 2),     # 18 taps: 8 B per lane; 10 column groups x 260 steps
              ((600, 63, 65), "db2", 1)]     # P odd: a dword per lane; 16 column groups x 300 steps
_WALK = {}


def walk_ref(case):
    if case not in _WALK:
        shape, wname, _ = case
        x = np.random.default_rng(sum(shape)).uniform(0.0, SCALE, shape).astype(np.float32)
        fwd64 = volume_ref.forward(x, wname, 1, "full")
        coef = [b.astype(np.float32) for b in fwd64]
        inv64 = volume_ref.inverse([c.astype(np.float64) for c in coef], shape, wname, 1, "full")
        for a in [x, inv64] + fwd64 + coef:
            a.setflags(write=False)
        _WALK[case] = (x, fwd64, coef, inv64)
    return _WALK[case]


@pytest.mark.parametrize("case", WALK_CASES, ids=["%dx%dx%d-%s" % (s + (w,)) for s, w, _ in WALK_CASES])
def test_depth_walks_of_several_steps(classes, case):
    shape, wname, width = case
    x, fwd64, coef, inv64 = walk_ref(case)
    W = classes[np.float32](x, wname, 1)
    got_width, seg_fwd, seg_inv = W.depth_schedule(1)
    assert got_width == width and seg_fwd >= 2 and seg_inv >= 2, (got_width, seg_fwd, seg_inv)
    W.forward()
    for num, g in enumerate(all_bands(W)):
        ref = fwd64[num]
        err, tol = float(np.abs(g.astype(np.float64) - ref).max()), 1.5e-6 * 2 * max(float(np.abs(ref).max()), 1.0)
        print(case, "band", num, "err %.3g tol %.3g" % (err, tol))
        assert g.shape == ref.shape and err <= tol, (case, num, err, tol)
    W.inverse()
    err = float(np.abs(W.image.astype(np.float64) - x).max())
    print(case, "round trip err %.3g" % err)
    assert err <= 7e-4 * SCALE / 255.0, (case, err)
    for num, c in enumerate(coef):
        W.set_coeff(c, num)
    W.inverse()
    err, tol = float(np.abs(W.image.astype(np.float64) - inv64).max()), 1.5e-6 * 2 * max(float(np.abs(inv64).max()), 1.0)
    print(case, "inverse alone err %.3g tol %.3g" % (err, tol))
    assert err <= tol, (case, err, tol)


# ---------------------------------------------------------------------------------------------------------- thresholds

THR_CASE = CASES[3]  # (64, 48, 40) db2: three levels


def _hip():
    lib = C.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return lib


def read_intermediate(W, level):
    """A_level of a level below the last: the depth-low half of band A of that level's plan, which sits right in front of the
    depth-high half 'daa' (include/pypwt_amd.h).  An intermediate, not a coefficient: read through the raw address."""
    W.synchronize()
    daa = W.coeff_device(volume_ref.num_of(level, "daa"))
    out = np.empty(daa.shape, dtype=daa.dtype)
    assert _hip().hipMemcpy(out.ctypes.data, C.c_void_p(daa.ptr - out.nbytes), out.nbytes, 2) == 0
    return out


@pytest.mark.parametrize("op", ["soft", "hard"])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("do_app", [0, 1])
def test_thresholds_bit_for_bit(classes, op, normalize, do_app):
    shape, wname, asked = THR_CASE
    r = ref_of(THR_CASE)
    L = r["levels"]
    assert L == 3
    W = classes[np.float32](r["x"], wname, asked)
    W.forward()
    before = all_bands(W)
    inter = [read_intermediate(W, l) for l in range(1, L)]
    # A_l of the fp64 composition: the intermediates are what the forward left there
    a = r["x"].astype(np.float64)
    for l in range(1, L):
        a = volume_ref.forward_level(a, wname, "full")["aaa"]
        assert np.abs(inter[l - 1] - a).max() <= 1e-4 * np.abs(a).max()  # the address is A_l's (no precision claim: a wrong one is off by 100 %)
    beta = 21.5
    getattr(W, op + "_threshold")(beta, do_app, normalize)
    want = volume_ref.threshold(before, L, op, beta, do_app, normalize)
    after = all_bands(W)
    for num, (g, w) in enumerate(zip(after, want)):
        assert ops_ref.same_bits(g, w), (op, normalize, do_app, num)
        if num > 0:
            assert not np.array_equal(g, before[num]), (num, "beta bites in every detail band")
    assert np.array_equal(after[0], before[0]) == (not (do_app and op == "soft"))  # (hard: every |A_L| is far above beta)
    for l in range(1, L):
        assert np.array_equal(read_intermediate(W, l), inter[l - 1]), ("intermediate A_%d was touched" % l)
    W.inverse()
    inv64 = volume_ref.inverse([b.astype(np.float64) for b in want], shape, wname, L, "full")
    inv32 = volume_ref.inverse(want, shape, wname, L, False)
    close32(W.image, inv64, inv32, L, (op, normalize, do_app, "inverse after threshold"))


@pytest.mark.parametrize("case", [CASES[2], CASES[3], CASES[8]], ids=[IDS[2], IDS[3], IDS[8]])
def test_norms(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked)
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
    case = CASES[3]
    shape, wname, asked = case
    r = ref_of(case)
    W = classes[np.float32](r["x"], wname, asked)
    lib = W._lib
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
    other = ref_of(CASES[3])["x"][::-1, ::-1, ::-1].copy()
    W.set_image(other)
    assert W.info()["state"] == _lib.STATE_INIT
    W.forward()
    L = r["levels"]
    ref64 = volume_ref.forward(other, wname, L, "full")
    ref32 = volume_ref.forward(other, wname, L, False)
    for num, g in enumerate(all_bands(W)):
        close32(g, ref64[num], ref32[num], L, ("second volume", num))
    # set_coeff of the approximation after an inverse makes the coefficients current again
    W.inverse()
    W.set_coeff(W.coeff_device(0), 0)  # its own buffer: nothing is copied
    assert W.info()["state"] == _lib.STATE_FORWARD
    W.hard_threshold(5.0)
    W.inverse()


def test_two_volumes_with_different_wavelets_alive_at_once(classes):
    a, b = CASES[1], CASES[4]
    ra, rb = ref_of(a), ref_of(b)
    Wa = classes[np.float32](ra["x"], a[1], a[2])
    Wb = classes[np.float32](rb["x"], b[1], b[2])
    Wa.forward()
    Wb.forward()
    for W, r, case in ((Wb, rb, b), (Wa, ra, a)):
        for num, g in enumerate(all_bands(W)):
            close32(g, r["fwd64"][num], r["fwd32"][num], r["levels"], (case, "alive together", num))


def test_input_from_a_torch_tensor_on_the_device(classes):
    import torch
    case = CASES[4]
    shape, wname, asked = case
    r = ref_of(case)
    t = torch.from_numpy(r["x"].copy()).to("cuda")
    W = classes[np.float32](t, wname, asked)
    assert np.array_equal(W.image, r["x"])
    W.forward()
    for num, g in enumerate(all_bands(W)):
        close32(g, r["fwd64"][num], r["fwd32"][num], r["levels"], (case, "torch", num))
    # device views and device sources
    view = torch.as_tensor(W.coeff_device(0), device="cuda")
    W.synchronize()
    assert np.array_equal(view.cpu().numpy(), W.coeff_only(0))
    t2 = (t * 0.5).contiguous()
    W.set_image(t2)
    torch.cuda.synchronize()
    assert np.array_equal(W.image, r["x"] * np.float32(0.5))
    img = torch.as_tensor(W.image_device, device="cuda")
    assert tuple(img.shape) == shape and np.array_equal(img.cpu().numpy(), W.image)


# ---------------------------------------------------------------------------------------------------------------- fp64

@pytest.mark.parametrize("case", CASES64, ids=IDS64)
def test_fp64_forward_inverse_round_trip(classes, case):
    shape, wname, asked = case
    r = ref_of(case)
    L = r["levels"]
    x = r["x"].astype(np.float64)
    W = classes[np.float64](x, wname, asked)
    assert W.levels == L
    W.forward()
    for num, g in enumerate(all_bands(W)):
        ref = r["fwd64"][num]
        assert g.dtype == np.float64 and g.shape == ref.shape
        assert np.abs(g - ref).max() <= 1e-12 * max(1.0, float(np.abs(ref).max())), (case, num)
    W.inverse()
    back = volume_ref.inverse(r["fwd64"], shape, wname, L, "full")
    assert np.abs(W.image - back).max() <= 1e-12 * max(1.0, float(np.abs(back).max())), case
    # the inverse alone, from coefficients that are not a transform of anything
    coef = [c.astype(np.float64) for c in r["coef"]]
    for num, c in enumerate(coef):
        W.set_coeff(c, num)
    for num, c in enumerate(coef):
        assert np.array_equal(W.coeff_only(num), c)
    W.inverse()
    assert np.abs(W.image - r["inv64"]).max() <= 1e-12 * max(1.0, float(np.abs(r["inv64"]).max())), case
    # thresholds and norms in fp64
    W.set_image(x)
    W.forward()
    before = all_bands(W)
    n = sum(b.size for b in before)
    n1, n2 = float(sum(np.abs(b).sum() for b in before)), float(sum((b * b).sum() for b in before))
    g1, g2 = W.norms()
    assert (g1, g2) == (W.norm1(), W.norm2sq())
    # n * 2^-53 for the reordered sum, and one more rounding per term for the squares formed in fp64
    assert abs(g1 - n1) <= n * 2.0 ** -53 * n1 and abs(g2 - n2) <= (n + 2) * 2.0 ** -53 * n2, (g1, n1, g2, n2)
    W.soft_threshold(17.25, 1, 1)
    for num, (g, w) in enumerate(zip(all_bands(W), volume_ref.threshold(before, L, "soft", 17.25, 1, 1))):
        assert ops_ref.same_bits(g, w), (case, num)


# ------------------------------------------------------------------------------------------ every name of the wavelet table
# The cases above are all orthogonal (rec is dec reversed): a volume that handed the wrong one of its dec / rec banks to a pass, or
# indexed it mirrored, would pass them.  Every name of the table goes through a volume here -- bior* and rbio* are the first
# biorthogonal ones --, one level, with the helpers and bounds of the tests above.  (13, 10, 14): planes of 140 samples, the wide
# access in fp32; (6, 9, 11): planes of 99 samples, one column per lane, a depth below most of these filters' lengths.
NAMES = list(oracle.filter_table()["order"])
BIORTHOGONAL = [w for w in NAMES if w[:4] in ("bior", "rbio", "coif")]
NAMES64 = ["bior3.9", "rbio6.8", "coif2"]
WIDE_SHAPE, NARROW_SHAPE = (13, 10, 14), (6, 9, 11)


def name_case(classes, dtype, shape, wname, width):
    """One level of `wname` on `shape`: the forward against the composition, then the inverse alone from random coefficients.  A name
    whose table length is odd is refused with PDWT_ERR_UNSUPPORTED (the depth kernels are built for even lengths)."""
    case = (shape, wname, 1)
    hlen = volume_ref.hlen_of(wname)
    if hlen & 1:
        with pytest.raises(NotImplementedError):
            classes[dtype](np.zeros(shape, dtype=dtype), wname, 1)
        return
    r = ref_of(case)
    assert r["levels"] == 1
    W = classes[dtype](r["x"].astype(dtype), wname, 1)
    assert (W.levels, W.hlen, W.nbands) == (1, hlen, 8)
    assert W.depth_schedule(1)[0] == width, (case, W.depth_schedule(1))
    W.forward()
    for num, g in enumerate(all_bands(W)):
        if dtype == np.float32:
            close32(g, r["fwd64"][num], r["fwd32"][num], 1, (case, "band", num))
        else:
            ref = r["fwd64"][num]
            assert g.dtype == np.float64 and g.shape == ref.shape
            assert np.abs(g - ref).max() <= 1e-12 * max(1.0, float(np.abs(ref).max())), (case, num)
    for num, c in enumerate(r["coef"]):
        W.set_coeff(c.astype(dtype), num)
    W.inverse()
    if dtype == np.float32:
        close32(W.image, r["inv64"], r["inv32"], 1, (case, "inverse"))
    else:
        assert np.abs(W.image - r["inv64"]).max() <= 1e-12 * max(1.0, float(np.abs(r["inv64"]).max())), case


def test_the_table_has_72_names_and_the_biorthogonal_ones_are_among_them():
    assert len(NAMES) == 72 and len(BIORTHOGONAL) == 33
    assert sum(w.startswith("bior") for w in NAMES) == 14 and sum(w.startswith("rbio") for w in NAMES) == 14


@pytest.mark.parametrize("wname", NAMES)
def test_every_wavelet_name_through_a_volume(classes, wname):
    hlen = volume_ref.hlen_of(wname)
    name_case(classes, np.float32, WIDE_SHAPE, wname, 4 if hlen <= 16 else 2)


@pytest.mark.parametrize("wname", BIORTHOGONAL)
def test_biorthogonal_and_coiflet_names_below_their_length(classes, wname):
    name_case(classes, np.float32, NARROW_SHAPE, wname, 1)


@pytest.mark.parametrize("shape", [WIDE_SHAPE, NARROW_SHAPE], ids=["13x10x14", "6x9x11"])
@pytest.mark.parametrize("wname", NAMES64)
def test_fp64_biorthogonal_names(classes, wname, shape):
    hlen = volume_ref.hlen_of(wname)
    name_case(classes, np.float64, shape, wname, (2 if hlen <= 16 else 1) if shape == WIDE_SHAPE else 1)
