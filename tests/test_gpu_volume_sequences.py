"""Model check of long-lived volume handles (`pytest -m gpu`): the call sequences of tests/volume_model.py on `pdwt_volume_*`
handles through the C ABI (V1, V2, V3) and through `Wavelets3D` / `Wavelets3D64` (V4), decimated and stationary, compared call by
call with the eager host model of that module.  tests/test_volume_model_cpu.py checks the model, the sequences' coverage and that
the comparator used here catches planted ordering defects.

After EVERY call the return value, the state and the shift equal the model's, what the call returns is compared at the bound the
operator's own test file uses, and the image, all 1 + 7 L sub-bands (raw reads through pdwt_volume_coeff_ptr, legal in every
state) and the twin's sub-bands equal the model's bit for bit.  The model is re-synchronised only where the library computes in
floating point across many terms -- forward, inverse, cycle_spin, add_wavelet, group_soft_threshold --: there the result is checked
against the bound and then adopted.

Those reads wait for the volume's stream after every call.  So every V1 sequence runs a second time on fresh handles with nothing
read back in between (run_blind) and must leave the same bits as the watched run -- state, shift, image, sub-bands, the twin's, every
result slot: what an operator finds in the select workspace, the staging buffer or another handle's stream while the previous
call is still running is seen only there.

Bounds (tests/volume_model.py: transform_bound, group_bound, table_bounds; none of them is new):
  forward / inverse   fp32: max(1.5e-6 (1 + L) max(max |ref64|, 1), 2 max |fp32 composition - fp64 composition|) per sub-band / on the
                      image, against the fp64 composition (tests/test_gpu_volume.py, test_gpu_volume_swt.py: tol32); the second term
                      is measured on the reference pair and scales with whatever a sequence hands the volume; fp64: 1e-12 max(1, max |ref|)
  cycle_spin          tests/volume_spin_ref.py: K_TOL = 4 times max |fp32 composition - fp64-accumulated composition|; fp64 1e-12 max |ref|;
                      the sub-bands it leaves behind (the last shift's, after its threshold: "spin_bands") at the forward's bound
  soft / hard / linf / shrink / threshold_bands / keep, every getter and setter: bit for bit
  group               5e-6 (fp64: 8 * 2^-52) max(max |ref band|, 1);  add_wavelet  one ulp of the reference (tests/test_gpu_volume_prox.py)
  norms               n 2^-53 relative (tests/test_gpu_volume.py::test_norms);  group_norm, band_stats  2 n 2^-53 relative
  estimate_sigma, select: exact;  denoise: sigma exact, the table by check_table's rule of tests/test_gpu_volume_ops.py, then the sweep
                      bit for bit with the DEVICE's table.  As there, a sub-band whose mean square is within the sum bound of the
                      max(., eps) edge is left out, one per table at most (asserted; the count is printed as "left-out")

The lines starting VSEQ are profiles/volume_sequences.txt.
"""
import contextlib
import ctypes as C
import io
import time

import numpy as np
import pytest

import volume_model as vm
import volume_spin_ref
from oracle import oracle

pytestmark = pytest.mark.gpu

RATIOS = ("forward", "inverse", "cycle_spin", "spin_bands", "group", "add", "norms", "group_norm", "band_stats", "table")
WORST = {}
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def built():
    oracle.build()


# --------------------------------------------------------------------------------------------------------------- the C ABI
class AbiVolume(object):
    """One volume handle of the library, driven through ctypes with the calls of volume_model.KINDS."""

    def __init__(self, spec, image, spinning=0):
        from pypwt_amd import _lib
        self._lib = _lib
        self.spec = spec
        self.lib = lib = _lib.load("f64" if spec.prec == "f64" else "f32")
        self.h = self.helper = None
        self.quiet = False  # True: nothing is read back that the call itself does not hand over (see run_blind)
        h = _lib.handle_t()
        img = np.ascontiguousarray(image, dtype=spec.dt)
        create = lib.pdwt_volume_create_swt if spec.swt else lib.pdwt_volume_create
        rc = create(img.ctypes.data, spec.shape[0], spec.shape[1], spec.shape[2], spec.wname.encode(), spec.asked, 1, -1, None, C.byref(h))
        assert rc == 0 and h.value, _lib.last_error(lib)
        self.h = h
        L = C.c_int()
        assert lib.pdwt_volume_get_info(h, None, None, None, C.byref(L), None, None) == 0
        assert L.value == spec.levels and lib.pdwt_volume_is_swt(h) == spec.swt, "the table's levels are not the library's"
        self.shapes = []
        for num in range(spec.nbands):
            d, r, c = C.c_int(), C.c_int(), C.c_int()
            assert lib.pdwt_volume_coeff_count(h, num, C.byref(d), C.byref(r), C.byref(c)) == d.value * r.value * c.value
            self.shapes.append((d.value, r.value, c.value))
        assert self.shapes == [tuple(s) for s in spec.band_shapes()]
        if spec.segments:
            for l in range(1, spec.levels + 1):
                assert lib.pdwt_volume_set_depth_segments(h, l, spec.segments, spec.segments) == 0, _lib.last_error(lib)
        if spinning:
            assert lib.pdwt_volume_set_cycle_spinning(h, 1, int(spinning)) == 0
        # a plan of the same library, for pdwt_copy alone: host data to a device pointer of the volume (the in-place setters)
        p = _lib.handle_t()
        assert lib.pdwt_create(None, 8, 8, b"haar", 1, 1, 1, 0, 0, 2, C.byref(p)) == 0, _lib.last_error(lib)
        self.helper = p

    def close(self):
        if self.h is not None:
            self.lib.pdwt_volume_destroy(self.h)
        if self.helper is not None:
            self.lib.pdwt_destroy(self.helper)
        self.h = self.helper = None

    def last_error(self):
        return " (%s)" % self._lib.last_error(self.lib)

    def state(self):
        st = C.c_int(-1)
        assert self.lib.pdwt_volume_get_info(self.h, None, None, None, None, None, C.byref(st)) == 0
        return st.value

    def shift(self):
        v = (C.c_int * 3)()
        assert self.lib.pdwt_volume_current_shift(self.h, v) == 0
        return tuple(int(x) for x in v)

    def image(self):
        out = np.empty(self.spec.shape, dtype=self.spec.dt)
        assert self.lib.pdwt_volume_get_image(self.h, out.ctypes.data) == out.size
        return out

    def read(self, ptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert ptr and self.lib.pdwt_volume_read(self.h, out.ctypes.data, C.c_void_p(int(ptr)), out.nbytes) == 0, self.last_error()
        return out

    def raw(self):
        """every sub-band through its device pointer: legal in every state"""
        return [self.read(self.lib.pdwt_volume_coeff_ptr(self.h, num), shp, self.spec.dt) for num, shp in enumerate(self.shapes)]

    def write(self, ptr, data):
        """host data to a device pointer of the volume, behind the library's back"""
        assert ptr and self.lib.pdwt_volume_synchronize(self.h) == 0
        assert self.lib.pdwt_copy(self.helper, C.c_void_p(int(ptr)), data.ctypes.data, data.size, 1) == 0, self.last_error()

    def slots(self):
        st, sg, tb = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.pdwt_volume_adaptive_slots(self.h, C.byref(st), C.byref(sg), C.byref(tb))
        return rc, st.value, sg.value, tb.value

    def sparsify(self):
        th, kp = C.c_void_p(), C.c_void_p()
        rc = self.lib.pdwt_volume_sparsify_slots(self.h, C.byref(th), C.byref(kp))
        if rc != 0:
            return rc, None
        return rc, (self.read(th.value, (1,), self.spec.dt), self.read(kp.value, (1,), np.uint64))

    def call(self, op, twin):
        """(return value, what the call hands the host or None)"""
        lib, h, s = self.lib, self.h, self.spec
        k, a = op[0], op[1:]
        nb = s.nbands
        if self.quiet and (k in vm.READERS or k in ("raw_read", "current_shift")):
            return 0, None
        if k == "forward":
            return lib.pdwt_volume_forward(h), None
        if k == "inverse":
            return lib.pdwt_volume_inverse(h), None
        if k == "soft":
            return lib.pdwt_volume_soft_threshold(h, a[0], a[1], a[2]), None
        if k == "hard":
            return lib.pdwt_volume_hard_threshold(h, a[0], a[1], a[2]), None
        if k == "group":
            return lib.pdwt_volume_group_soft_threshold(h, a[0], a[1], a[2]), None
        if k == "linf":
            return lib.pdwt_volume_proj_linf(h, a[0], a[1]), None
        if k == "shrink":
            return lib.pdwt_volume_shrink(h, a[0], a[1]), None
        if k == "norms":
            out = (C.c_double * 2)(7.0, 7.0)
            return lib.pdwt_volume_norms(h, out), (out[0], out[1])
        if k == "group_norm":
            out = C.c_double(7.0)
            return lib.pdwt_volume_group_norm(h, a[0], C.byref(out)), out.value
        if k == "add_dst":
            return lib.pdwt_volume_add_wavelet(h, twin.h, a[0]), None
        if k == "add_src":
            return lib.pdwt_volume_add_wavelet(twin.h, h, a[0]), None
        if k == "get_image":
            out = np.full(s.shape, 7.0, dtype=s.dt)
            return int(lib.pdwt_volume_get_image(h, out.ctypes.data)), out
        if k == "get_coeff":
            out = np.full(self.shapes[a[0]], 7.0, dtype=s.dt)
            return int(lib.pdwt_volume_get_coeff(h, out.ctypes.data, a[0])), out
        if k == "raw_read":
            return 0, self.raw()
        if k == "set_image":
            img = s.image(a[0])
            if a[1]:  # in place: the data is written through the handle's own pointer, which is then passed as a device source
                ptr = lib.pdwt_volume_image_ptr(h)
                self.write(ptr, img)
                return lib.pdwt_volume_set_image(h, C.c_void_p(ptr), 1), None
            return lib.pdwt_volume_set_image(h, img.ctypes.data, 0), None
        if k == "set_coeff":
            band = s.band(a[0], a[1])
            if a[2]:
                ptr = lib.pdwt_volume_coeff_ptr(h, a[0])
                self.write(ptr, band)
                return lib.pdwt_volume_set_coeff(h, C.c_void_p(ptr), a[0], 1), None
            return lib.pdwt_volume_set_coeff(h, band.ctypes.data, a[0], 0), None
        if k == "circshift":
            return lib.pdwt_volume_circshift(h, a[0], a[1], a[2]), None
        if k == "spin_on":
            return lib.pdwt_volume_set_cycle_spinning(h, 1, a[0]), None
        if k == "spin_off":
            return lib.pdwt_volume_set_cycle_spinning(h, 0, 0), None
        if k == "current_shift":
            return 0, self.shift()
        if k == "cycle_spin":
            variant, mode, value, do_app, normalize, nshifts = a
            sh = np.ascontiguousarray(volume_spin_ref.lattice(nshifts), dtype=np.int32)
            sp = sh.ctypes.data_as(C.POINTER(C.c_int))
            opn = 0 if mode == "soft" else 1
            if variant == "global":
                return lib.pdwt_volume_cycle_spin_async(h, nshifts, sp, opn, float(value), do_app, normalize, -1, None, 1), None
            sigma = C.c_double(value)
            return lib.pdwt_volume_cycle_spin_async(h, nshifts, sp, opn, 0.0, 0, 0, 1, C.byref(sigma), 1), None
        if k == "band_stats":
            rc = lib.pdwt_volume_band_stats_async(h, None)
            return rc, (self.read(self.slots()[1], (nb, 2), np.float64) if rc == 0 and not self.quiet else None)
        if k == "estimate_sigma":
            rc = lib.pdwt_volume_estimate_sigma_async(h, a[0], None)
            return rc, (self.read(self.slots()[2], (1,), np.float64) if rc == 0 and not self.quiet else None)
        if k == "threshold_bands":
            T = s.table(a[0], a[2])
            return lib.pdwt_volume_threshold_bands(h, 0 if a[1] == "soft" else 1, T.ctypes.data, 0), None
        if k == "denoise":
            method, mode, sigma, skip = a
            sg = C.c_double(sigma if sigma is not None else 0.0)
            rc = lib.pdwt_volume_denoise_async(h, 0 if method == "BayesShrink" else 1, 0 if mode == "soft" else 1,
                                               C.byref(sg) if sigma is not None else None, skip)
            if rc != 0 or self.quiet:
                return rc, None
            _, _, p_sigma, p_table = self.slots()
            return rc, (self.read(p_sigma, (1,), np.float64), self.read(p_table, (nb,), s.dt))
        if k == "select":
            rc = lib.pdwt_volume_select_magnitude_async(h, a[0], a[1], None, None)
            return rc, (self.sparsify()[1] if rc == 0 and not self.quiet else None)
        if k == "keep":
            rc = lib.pdwt_volume_keep_largest_async(h, a[0], a[1])
            return rc, (self.sparsify()[1] if rc == 0 and not self.quiet else None)
        if k == "norms_async":
            rc = lib.pdwt_volume_norms_async(h, None)
            return rc, (self.read(self.slots()[1] + 2 * nb * 8, (2,), np.float64) if rc == 0 and not self.quiet else None)
        if k == "last_sparsify":
            return self.sparsify()
        if k in vm.READERS:
            rc, p_stats, p_sigma, p_table = self.slots()
            if rc != 0:
                return rc, None
            if k == "read_sigma":
                return rc, self.read(p_sigma, (1,), np.float64)
            if k == "read_band_stats":
                return rc, self.read(p_stats, (nb, 2), np.float64)
            if k == "read_norms":
                return rc, self.read(p_stats + 2 * nb * 8, (2,), np.float64)
            return rc, (self.read(p_sigma, (1,), np.float64), self.read(p_table, (nb,), s.dt))
        raise ValueError(op)


def run_ops(spec, ops, seed=0, stats=None, at_end=None):
    """What a failing sequence prints calls this."""
    oracle.build()
    return vm.run_sequence(spec, ops, AbiVolume, seed, stats, at_end=at_end)


def snapshot(v, twin):
    """Everything a handle holds that a caller can reach: state, shift, image, sub-bands, the twin's, and the result slots."""
    out = {"state": np.array([v.state()]), "shift": np.array(v.shift()), "image": v.image()}
    for num, b in enumerate(v.raw()):
        out["band %d" % num] = b
    for num, b in enumerate(twin.raw()):
        out["twin band %d" % num] = b
    if not v.spec.swt:
        nb = v.spec.nbands
        _, p_stats, p_sigma, p_table = v.slots()
        out["stats and norms"] = v.read(p_stats, (nb + 1, 2), np.float64)
        out["sigma"], out["table"] = v.read(p_sigma, (1,), np.float64), v.read(p_table, (nb,), v.spec.dt)
        out["sparsify threshold"], out["kept"] = v.sparsify()[1]
    return out


def run_blind(spec, ops, seed, wait=False):
    """The same calls on fresh handles with NOTHING read back in between -- the comparator's reads wait for the volume's stream
    after every call, which would hide an operator that reuses the select workspace, the pinned staging buffer or a result slot
    before the previous one is done with it.  What is left are the waits of the calls themselves (the blocking getters and
    norms, host sources, the behind-the-back writes of the in-place setters).  `wait`: both streams are waited for after every
    call instead.  Returns the snapshot at the end."""
    image = spec.image(100 + seed)
    v = twin = None
    try:
        v, twin = AbiVolume(spec, image, spec.cycle), AbiVolume(spec, image)
        v.quiet = twin.quiet = True
        assert v.call(("forward",), None)[0] == 0 and twin.call(("forward",), None)[0] == 0
        for op in ops:
            v.call(op, twin)
            if wait:
                assert v.lib.pdwt_volume_synchronize(v.h) == 0 and v.lib.pdwt_volume_synchronize(twin.h) == 0
        return snapshot(v, twin)
    finally:
        for s in (v, twin):
            if s is not None:
                s.close()


def report(tag, spec, stats):
    for k in RATIOS:
        WORST[k] = max(WORST.get(k, 0.0), stats[k])
    assert all(stats[k] <= 1.0 for k in RATIOS)
    print("VSEQ %s %-26s calls %d refused %d left-out %d | largest seen/bound: %s" % (
        tag, spec.name, stats["calls"], stats["refused"], stats["left_out"], " ".join("%s %.3f" % (k, stats[k]) for k in RATIOS)))


# --------------------------------------------------------------------------------------------------------------- V1
@pytest.mark.parametrize("spec", vm.VOLUMES, ids=lambda s: s.name)
def test_v1_random_sequences_through_the_c_abi(spec):
    stats = vm.new_stats()
    for seed in vm.SEEDS:
        ops = vm.sequences()[(spec.name, seed)]
        watched = {}
        run_ops(spec, ops, seed, stats, at_end=lambda v, twin: watched.update(snapshot(v, twin)))
        # ... and once more with no host wait between the calls: the same bits everywhere, the result slots included
        blind = run_blind(spec, ops, seed)
        assert sorted(blind) == sorted(watched)
        for key in sorted(watched):
            vm.same_bits(blind[key], watched[key], "%s, seed %d, without reads in between: %s" % (spec.name, seed, key))
    report("V1", spec, stats)


# volumes whose forward keeps the stream busy for longer than the host needs to enqueue the next two calls (a million voxels and
# more), and the small one the random sequences found it on
OVERTAKEN = [vm.VolumeSpec("swt-64x128x128-haar-L2", (64, 128, 128), "haar", 2, swt=1),
             vm.VolumeSpec("dwt-128x128x128-db2-L2", (128, 128, 128), "db2", 2), vm.spec_named("swt-5x7x11-haar-L2")]


@pytest.mark.parametrize("spec", OVERTAKEN, ids=lambda s: s.name)
def test_add_wavelet_holds_the_sources_later_work_until_it_has_read(spec):
    """`twin.add_wavelet(volume)` and then, with no host wait, a threshold of `volume`: the sum runs on the twin's stream and was
    ordered after the volume's earlier work only, so the threshold -- on the volume's own stream -- overtook it and the twin
    received coefficients that were thresholded in part (swt-5x7x11-haar-L2, seed 2, calls 20-23: 256 of the 385 values of the
    twin's sub-band 1 differed from the run that reads after every call).  The loop in the README does this with `D.shrink` after
    `X.add_wavelet(D)`.  pdwt_volume_add_wavelet now makes the source's stream wait for the sum's read.
    Here four forwards are queued first, so that the sum (which waits for them) and the sweep behind them become ready together;
    the sweeps change every coefficient they reach."""
    busy = [("forward",)] * 4
    ops = busy + [("add_src", 1.0), ("shrink", 3.0, 1)] + busy + [("add_src", -1.25), ("soft", 40.0, 1, 0), ("add_dst", 0.5), ("linf", 3.0, 1)]
    waited, blind = run_blind(spec, ops, 7, wait=True), run_blind(spec, ops, 7)
    assert sorted(blind) == sorted(waited)
    for key in sorted(waited):
        vm.same_bits(blind[key], waited[key], "without a wait in between: " + key)


# --------------------------------------------------------------------------------------------------------------- V2
def canned(spec):
    """The orderings the comments of volume.cpp name, independent of any seed.  A stationary volume refuses some of the calls;
    the rest of each ordering still runs."""
    return [
        # a threshold, inverse, the re-arm from the handle's own pointer (inverse_levels does the same to every level plan), again
        ("soft", 40.0, 0, 0), ("inverse",), ("set_coeff", 0, 901, 1), ("hard", 12.0, 0, 0), ("inverse",),
        # forwards in a row on a spinning handle: the shift is the sum, then zero
        ("set_image", 902, 0), ("spin_on", 77), ("forward",), ("forward",), ("current_shift",), ("inverse",), ("current_shift",),
        # set_image zeroes the shift
        ("forward",), ("set_image", 903, 1), ("current_shift",),
        # circshift after an inverse: state INIT, the getters are legal again, and the coefficients are still the old ones
        ("forward",), ("inverse",), ("circshift", 1, -2, 3), ("get_coeff", 1), ("forward",), ("inverse",), ("spin_off",),
        # the radix-select workspace between the noise estimate and the K-term operators
        ("forward",), ("estimate_sigma", 1), ("keep", spec.swept(0) // 4, 0), ("estimate_sigma", 1), ("read_sigma",),
        # the sigma slot between cycle_spin(sigma=..) and the estimate of the next denoise
        ("inverse",), ("cycle_spin", "visu", "soft", vm.SPIN_SIGMA, 0, 0, 2), ("read_sigma",), ("forward",), ("denoise", "BayesShrink", "soft", None, 1),
        # the coefficients cycle_spin leaves behind can be re-armed
        ("set_image", 904, 0), ("cycle_spin", "global", "hard", 40.0, 1, 0, 3), ("set_coeff", 0, 905, 0), ("soft", 20.0, 1, 1), ("inverse",),
        # both operands of add_wavelet, then a forward of each: the intermediates A_1 .. A_{L-1} it scaled do not show
        ("forward",), ("add_src", 0.5), ("add_dst", -1.25), ("twin_forward",), ("forward",), ("raw_read",),
        # thresholds in a row with other betas (a stationary volume stages its table through one pinned buffer)
        ("soft", 40.0, 0, 0), ("hard", 12.0, 1, 1), ("soft", 3.0, 1, 0), ("linf", 2.0, 1), ("shrink", 0.25, 0),
        # a host table directly after the device's own
        ("forward",), ("denoise", "VisuShrink", "hard", None, 0), ("threshold_bands", 906, "soft", 1), ("last_thresholds",), ("norms",),
        ("group", 30.0, 1, 0), ("group_norm", 1),
        # the pinned staging buffer: K, a given noise level, K again and another noise level, with nothing waiting in between
        ("forward",), ("keep", spec.swept(1) // 2, 1), ("denoise", "BayesShrink", "soft", vm.SPIN_SIGMA, 1), ("select", 5, 0),
        ("denoise", "VisuShrink", "hard", 2.5, 0), ("last_sparsify",), ("last_thresholds",), ("norms_async",), ("band_stats",), ("read_norms",),
        ("inverse",), ("read_band_stats",), ("get_coeff", 0),
    ]


@pytest.mark.parametrize("spec", vm.VOLUMES, ids=lambda s: s.name)
def test_v2_named_orderings_on_every_volume(spec):
    stats = run_ops(spec, canned(spec), 9)
    report("V2", spec, stats)
    if spec.swt:
        return
    # cycle_spin twice on the same image: the same bits (the two extra volumes and the level plans carry nothing over)
    v = AbiVolume(spec, spec.image(31))
    try:
        op = ("cycle_spin", "global", "soft", 40.0, 0, 1, 3)
        assert v.call(op, None)[0] == 0
        first, first_bands = v.image(), v.raw()
        assert v.call(("set_image", 31, 0), None)[0] == 0
        assert v.call(op, None)[0] == 0 and v.state() == vm.INVERSE
        vm.same_bits(v.image(), first, "cycle_spin again")
        for num, (g, w) in enumerate(zip(v.raw(), first_bands)):
            vm.same_bits(g, w, "cycle_spin again: sub-band %d" % num)
    finally:
        v.close()


# --------------------------------------------------------------------------------------------------------------- V3
@pytest.mark.parametrize("spec", vm.VOLUMES, ids=lambda s: s.name)
def test_v3_transforms_leave_their_inputs_alone(spec):
    """forward() does not write the image, inverse() writes none of the 1 + 7 L visible sub-bands (volume.hpp: the depth-low half
    of band A is an intermediate below the last level only), and six rounds on one handle give the first round's bits."""
    x = spec.image(41)
    v = AbiVolume(spec, x)  # (cycle spinning off: a spinning forward shifts the image)
    try:
        rounds = []
        for r in range(6):
            assert v.call(("set_image", 41, r % 2), None)[0] == 0
            vm.same_bits(v.image(), x, "set_image")
            assert v.call(("forward",), None)[0] == 0
            vm.same_bits(v.image(), x, "the image after forward()")
            bands = v.raw()
            assert v.call(("inverse",), None)[0] == 0
            img = v.image()
            for num, (g, w) in enumerate(zip(v.raw(), bands)):
                vm.same_bits(g, w, "sub-band %d after inverse()" % num)
            # the re-arm from the handle's own pointer moves nothing: the same image again
            ptr = v.lib.pdwt_volume_coeff_ptr(v.h, 0)
            assert v.lib.pdwt_volume_set_coeff(v.h, C.c_void_p(ptr), 0, 1) == 0 and v.state() == vm.FORWARD
            assert v.call(("inverse",), None)[0] == 0
            vm.same_bits(v.image(), img, "the image of a second inverse()")
            for num, (g, w) in enumerate(zip(v.raw(), bands)):
                vm.same_bits(g, w, "sub-band %d after the second inverse()" % num)
            rounds.append((bands, img))
        for r in range(1, 6):
            vm.same_bits(rounds[r][1], rounds[0][1], "the image of round %d" % (r + 1))
            for num, (g, w) in enumerate(zip(rounds[r][0], rounds[0][0])):
                vm.same_bits(g, w, "sub-band %d of round %d" % (num, r + 1))
    finally:
        v.close()


# --------------------------------------------------------------------------------------------------------------- V4
# how `Wavelets3D` turns PDWT_ERR_STATE down: these print the reference's warning and return, everything else raises
WARNS = ("inverse", "soft", "hard", "group", "linf", "shrink", "add_dst", "add_src", "threshold_bands", "denoise", "keep")


class ClassVolume(object):
    """A `Wavelets3D` / `Wavelets3D64` behind the subject's interface: methods only; what they raise or print stands for the code."""

    def __init__(self, spec, image, spinning=0):
        import pypwt_amd
        self.pdwt_error = pypwt_amd._lib.PdwtError
        self.spec = spec
        cls = pypwt_amd.Wavelets3D64 if spec.prec == "f64" else pypwt_amd.Wavelets3D
        self.W = W = cls(np.ascontiguousarray(image, dtype=spec.dt), spec.wname, spec.asked, do_swt=spec.swt)
        assert W.levels == spec.levels and [tuple(W.band_shape(n)) for n in range(W.nbands)] == [tuple(b) for b in spec.band_shapes()]
        if spec.segments:
            for l in range(1, spec.levels + 1):
                W._set_depth_segments(l, spec.segments, spec.segments)
        if spinning:
            W.set_cycle_spinning(1, spinning)
        self.message = ""

    def close(self):
        self.W.cleanup()

    def last_error(self):
        return " (%s)" % self.message

    def state(self):
        return self.W.info()["state"]

    def shift(self):
        return self.W.last_shift

    def image(self):
        return self.W.image

    def raw(self):
        W = self.W
        return [W._read(W._addr(W.coeff_device(num)), W.band_shape(num), self.spec.dt) for num in range(W.nbands)]

    def call(self, op, twin):
        k = op[0]
        out = io.StringIO()
        self.message = ""
        try:
            with contextlib.redirect_stdout(out):
                data = self._call(op, twin)
        except NotImplementedError as e:
            self.message = str(e)
            return vm.ERR_UNSUPPORTED, None
        except self.pdwt_error as e:
            self.message = str(e)
            assert k not in WARNS, "%s raised where the class warns: %s" % (k, e)
            return vm.ERR_STATE, None
        except RuntimeError as e:  # coeff_only after inverse(): "expected n values, got 0"
            self.message = str(e)
            assert k == "get_coeff" and "got 0" in str(e), (k, e)
            return 0, np.full(self.W.band_shape(op[1]), 7.0, dtype=self.spec.dt)
        if "Warning" in out.getvalue():
            self.message = out.getvalue().strip()
            assert k in WARNS, "%s warned where the class raises: %s" % (k, self.message)
            return vm.ERR_STATE, None
        if k in ("get_image", "get_coeff"):
            return data.size, data
        return 0, data

    def _call(self, op, twin):
        W, s = self.W, self.spec
        k, a = op[0], op[1:]
        if k == "forward":
            return W.forward()
        if k == "inverse":
            return W.inverse()
        if k == "soft":
            return W.soft_threshold(*a)
        if k == "hard":
            return W.hard_threshold(*a)
        if k == "group":
            return W.group_soft_threshold(*a)
        if k == "linf":
            return W.proj_linf(*a)
        if k == "shrink":
            return W.shrink(*a)
        if k == "norms":
            return W.norms()
        if k == "group_norm":
            return W.group_norm(a[0])
        if k == "add_dst":
            return W.add_wavelet(twin.W, a[0])
        if k == "add_src":
            return twin.W.add_wavelet(W, a[0])
        if k == "get_image":
            return W.image
        if k == "get_coeff":
            return W.coeff_only(a[0])
        if k == "set_image":
            W.set_image(s.image(a[0]))
            if a[1]:  # ... and once more from its own device view: nothing moves, the state and the shift are set again
                W.set_image(W.image_device)
            return None
        if k == "set_coeff":
            W.set_coeff(s.band(a[0], a[1]), a[0])
            if a[2]:
                W.set_coeff(W.coeff_device(a[0]), a[0])
            return None
        if k == "circshift":
            return W.circshift(*a)
        if k == "spin_on":
            W.set_cycle_spinning(1, a[0])
            return None
        if k == "spin_off":
            W.set_cycle_spinning(0)
            return None
        if k == "current_shift":
            return W.last_shift
        if k == "cycle_spin":
            variant, mode, value, do_app, normalize, nshifts = a
            if variant == "global":
                W.cycle_spin(n=nshifts, mode=mode, beta=value, do_threshold_appcoeffs=do_app, normalize=normalize)
            else:
                W.cycle_spin(n=nshifts, mode=mode, method="VisuShrink", sigma=value)
            return None
        if k == "band_stats":
            return W.read_band_stats(W.band_stats())
        if k == "estimate_sigma":
            return W.read_sigma(W.estimate_sigma(skip_zeros=bool(a[0])))
        if k == "threshold_bands":
            return W.threshold_bands(s.table(a[0], a[2]), a[1])
        if k == "denoise":
            W.denoise(method=a[0], sigma=a[2], mode=a[1], skip_zeros=bool(a[3]))
            return W.last_thresholds()
        if k == "select":
            W.select_magnitude(k=a[0], do_threshold_appcoeffs=a[1])
            return W.last_sparsify()
        if k == "keep":
            W.keep_largest(k=a[0], do_threshold_appcoeffs=a[1])
            return W.last_sparsify()
        if k == "norms_async":
            return np.array(W.read_norms(W.norms_device()))
        if k == "read_sigma":
            return W.read_sigma()
        if k == "read_band_stats":
            return W.read_band_stats()
        if k == "read_norms":
            return np.array(W.read_norms())
        if k == "last_thresholds":
            return W.last_thresholds()
        if k == "last_sparsify":
            return W.last_sparsify()
        raise ValueError(op)


@pytest.mark.parametrize("spec", vm.VOLUMES, ids=lambda s: s.name)
def test_v4_random_sequence_through_the_python_class(spec):
    stats = vm.run_sequence(spec, vm.sequences()[(spec.name, vm.CLASS_SEED)], ClassVolume, vm.CLASS_SEED)
    report("V4", spec, stats)


def test_report():
    """Closes the module: the largest seen / bound of every comparison over all volumes, and the module's wall time."""
    print("VSEQ all: largest seen/bound: %s | %d volumes x (%d C-ABI sequences + named orderings + 1 class sequence) of %d calls | %.0f s" % (
        " ".join("%s %.3f" % (k, WORST.get(k, 0.0)) for k in RATIOS), len(vm.VOLUMES), len(vm.SEEDS), vm.LENGTH, time.time() - T0))
    assert all(v <= 1.0 for v in WORST.values())
