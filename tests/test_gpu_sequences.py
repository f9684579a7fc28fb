"""Call sequences on long-lived plans, checked call by call against the eager host model of tests/plan_model.py (`pytest -m gpu`).

Every other GPU test has one shape: create a plan, forward(), at most one operator, inverse(), throw the plan away.  An iterative
solver keeps ONE plan and calls its entry points in any order, and that is where plan.cpp's lazy state lives: a soft threshold that
a separable 2D SWT plan defers into its inverse (`pending`) and the write-back such an inverse owes (`consumed`).

C1  seeded random sequences (plan_model.sequences(): conditions checked without a GPU by test_plan_model_cpu.py) on the plans of
    plan_model.PLANS, through the C ABI and through the Python classes.  After every call: return value and state equal the
    model's; whatever the call reads equals the model's BIT FOR BIT (test_gpu_ops_scale.py has the operators bit for bit), except
    where the project's own bound is wider (add_wavelet: one ulp, group_soft_threshold: 5e-6 / 8 x 2.15e-16 relative, the norms:
    2 n 2^-53 relative).  The model is re-synchronised at transforms only: forward() and inverse() are compared with the CPU
    oracle within the project's bounds (forward_bound / inverse_bound below name where each comes from) and the model then adopts
    the library's result.  Seeds 6 and 7 (8 through the classes) also draw the adaptive and K-term calls, the readers of their
    slots and take_band, under the bounds of tests/test_gpu_adaptive.py and tests/test_gpu_sparsify.py: the sums 2 n 2^-53 relative
    per entry, the noise levels, the select's threshold and count exact, the sweeps bit for bit, a denoise table by the rule of
    tests/adaptive_check.py (the model then adopts the device's table).
    Every C-ABI sequence runs a SECOND time on a fresh plan and clone with nothing read back between the calls (run_blind) and
    must leave the same bits everywhere a caller can look (snapshot): the watched run's reads wait for the plan's stream after
    every call, so only the blind run can see what a call finds while the previous one is still running.  The comparison is
    between two runs of the library: it shows an ordering defect, not a wrong result -- that is the watched run's part.
C2  fused = eager, bit for bit: on every separable 2D SWT plan of the dispatch table, inverse() with the threshold still pending
    (the `+soft` launches) against inverse() after it was materialised.
C3  transforms leave their inputs alone, on the whole dispatch table: forward() its image, inverse() the coefficients; and five
    more rounds on the same plan give round 1's bits.

Lines that start with "SEQ" carry the figures (run with -s).
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import ops_ref
import plan_model as pm
from adaptive_check import check_table, left_out_pairs, swept
from dispatch_cases import CASES as DISPATCH_CASES
from golden_util import reconstruction_tol
from oracle import oracle
from test_gpu_ops_scale import GROUP_SOFT_F64_MEASURED, Plan

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
WORST = {"forward": 0.0, "inverse": 0.0, "band_stats": 0.0}  # largest seen / bound of the comparisons with a bound, over the whole module


# --------------------------------------------------------------------------------------------------------------- the bounds
def forward_bound(spec, num, ref, image):
    """|library - oracle| of one band after forward()."""
    rmax = float(np.abs(ref).max())
    L = spec.levels
    if not spec.separable:  # test_gpu_ops.py::test_nonseparable_inverse_of_a_genuinely_nonseparable_bank_vs_oracle
        return 2e-5 * max(rmax, 1.0)
    if spec.prec == "f64":  # tools/soak.py: check64
        return 1e-12 * (1 + L) * max(1.0, rmax)
    # tools/soak.py: check / test_gpu_fuzz.py::test_fuzz_three_level_pyramid, stated for images of 0..255; a sequence may hand the
    # plan a reconstruction that exceeds 255 (add_wavelet, negative beta), so 255 is the image's magnitude where that is larger
    mag = max(255.0, float(np.abs(image).max()))
    return 2e-6 * (L + 1) * max(rmax, mag * 2.0 ** spec.level_of(num))


def inverse_bound(spec, bands, want):
    """|library - oracle| of the image after inverse() of the same coefficients."""
    wmax = float(np.abs(want).max())
    if not spec.separable:  # test_gpu_ops.py::test_nonseparable_inverse_of_a_genuinely_nonseparable_bank_vs_oracle
        return 3e-5 * max(wmax, 1.0)
    # test_gpu_dispatch.py::test_every_reachable_dispatch_pair_runs_and_matches_the_oracle: (2e-6 | 1e-11) (1 + L) 255 on the
    # coefficients of a 0..255 image.  A sequence's coefficients can be far larger (add_wavelet, set_coeff, a custom bank), so 255
    # is replaced by the magnitude of the coefficients brought to the image's scale (2^-l per 2D level, 2^(-l/2) in 1D) or of the
    # reconstruction where that is larger; the seen / bound ratio is reported
    g = 2.0 if spec.ndim == 2 else 2.0 ** 0.5
    mag = max([255.0, wmax] + [float(np.abs(b).max()) / g ** spec.level_of(k) for k, b in enumerate(bands)])
    return (1e-11 if spec.prec == "f64" else 2e-6) * (1 + spec.levels) * mag


def norms_bound(total):
    """relative: recursive summation over the swept (padded) length, tests/test_gpu_ops_scale.py: norms_bound"""
    return 2.0 * total * U53


def assert_same_bits(got, want, what):
    got = np.asarray(got).reshape(-1)
    want = np.asarray(want).reshape(-1)
    if not ops_ref.same_bits(got, want):
        bad = np.flatnonzero((got != want) | (np.signbit(got) != np.signbit(want)))
        raise AssertionError("%s: %d of %d values differ from the model, first at %d: %r != %r" % (
            what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def assert_close_bands(spec, got, want, kind, what):
    """add_wavelet: one ulp (test_gpu_ops_scale.py B3); group_soft_threshold: its bound there (B2)"""
    for k, (g, r) in enumerate(zip(got, want)):
        g, r = g.reshape(-1), r.reshape(-1)
        if kind == "add":
            assert float((np.abs(g - r) / np.spacing(np.abs(r))).max()) <= 1.0, (what, k)
        else:
            tol = 5e-6 if spec.dt is np.float32 else 8 * GROUP_SOFT_F64_MEASURED
            err = float(np.abs(g.astype(np.longdouble) - r.astype(np.longdouble)).max()) / max(float(np.abs(r).max()), 1.0)
            assert err <= tol, (what, k, err)


# --------------------------------------------------------------------------------------------------------------- the C ABI
class AbiPlan(object):
    """One plan of the library, driven through ctypes with the calls of plan_model.KINDS."""

    def __init__(self, spec, image=None, handle=None, lib=None):
        from pypwt_amd import _lib
        self.spec = spec
        self.lib = lib or _lib.load("f64" if spec.prec == "f64" else "f32")
        self.parent = None
        self.quiet = False  # True: nothing is read back that the call itself does not hand over (see run_blind)
        self.tables = []    # device tables of threshold_bands: they live as long as the plan (freeing one waits for the device)
        if handle is not None:
            self.h = handle
        else:
            h = _lib.handle_t()
            img = np.ascontiguousarray(image, dtype=spec.dt)
            rc = self.lib.pdwt_create_batched(img.ctypes.data, spec.batch, spec.shape[0], spec.shape[1], spec.wname.encode(), spec.levels, 1,
                                              spec.separable, spec.cycle, spec.swt, spec.ndim, -1, None, C.byref(h))
            assert rc == 0, self.lib.pdwt_last_error()
            self.h = h
            if spec.bound:  # the image IS band 0 of a one-level 128 x 128 plan (pdwt_bind_image)
                assert spec.shape == (64, 64) and spec.batch == 1
                p = _lib.handle_t()
                assert self.lib.pdwt_create_batched(None, 1, 128, 128, b"db2", 1, 1, 1, 0, 0, 2, -1, None, C.byref(p)) == 0
                self.parent = p
                # a plan created without an image zeroes its arena on ITS stream and waits for nothing: this plan writes the image
                # into that arena on another stream, so the zeroing has to be over first (seen once: a forward of zeros)
                assert self.lib.pdwt_synchronize(p) == 0
                assert self.lib.pdwt_bind_image(self.h, C.c_void_p(self.lib.pdwt_coeff_ptr(p, 0))) == 0
                assert self.lib.pdwt_image_ptr(self.h) == self.lib.pdwt_coeff_ptr(p, 0)
                assert self.lib.pdwt_set_image(self.h, img.ctypes.data, 0) == 0
        info, st, b = _lib.PdwtInfo(), C.c_int(), C.c_int()
        assert self.lib.pdwt_get_info(self.h, C.byref(info), None, None, C.byref(st), C.byref(b)) == 0
        assert (info.nlevels, b.value, info.Nr, info.Nc) == (spec.levels, spec.batch) + spec.shape, "the table's levels are not clamped"
        nb = spec.nbands
        offs = (C.c_longlong * nb)()
        self.total = int(self.lib.pdwt_coeff_region(self.h, offs, nb))
        self.offs = [int(o) for o in offs]
        self.elems = [int(self.lib.pdwt_coeff_count(self.h, k, None, None)) for k in range(nb)]

    def close(self):
        for h in (self.h, self.parent):
            if h is not None:
                self.lib.pdwt_destroy(h)
        self.h = self.parent = None
        self.tables = []

    def last_error(self):
        return self.lib.pdwt_last_error()

    def read(self, addr, shape, dtype):
        """device memory of the plan through pdwt_copy: waits for the plan's stream"""
        from pypwt_amd.wavelets import _read_device
        return _read_device(self.lib, self.h, addr, shape, dtype)

    def slots(self):
        """the three adaptive slots and the two sparsify slots (the getters allocate the workspace where no call has)"""
        s = self.spec
        st, sg, tb, th, kp = (C.c_void_p() for _ in range(5))
        assert self.lib.pdwt_adaptive_slots(self.h, C.byref(st), C.byref(sg), C.byref(tb)) == 0, self.last_error()
        assert self.lib.pdwt_sparsify_slots(self.h, C.byref(th), C.byref(kp)) == 0, self.last_error()
        return {"band stats": self.read(st.value, (s.nbands, s.batch, 2), np.float64), "sigma": self.read(sg.value, (s.batch,), np.float64),
                "table": self.read(tb.value, (s.nbands, s.batch), s.dt), "sparsify threshold": self.read(th.value, (s.batch,), s.dt),
                "kept": self.read(kp.value, (s.batch,), np.uint64)}

    def norms_slot(self):
        from pypwt_amd.wavelets import _read_norms
        return np.array(_read_norms(self.lib, self.h, None))

    def state(self):
        st = C.c_int()
        assert self.lib.pdwt_get_info(self.h, None, None, None, C.byref(st), None) == 0
        return st.value

    def shift(self):
        sr, sc = C.c_int(), C.c_int()
        assert self.lib.pdwt_current_shift(self.h, C.byref(sr), C.byref(sc)) == 0
        return sr.value, sc.value

    def image(self):
        s = self.spec
        out = np.empty((s.batch,) + s.shape, dtype=s.dt)
        assert self.lib.pdwt_get_image(self.h, out.ctypes.data) == out.size
        return out

    def image_raw(self):
        """the image through its device pointer"""
        s = self.spec
        out = np.empty((s.batch,) + s.shape, dtype=s.dt)
        ptr = self.lib.pdwt_image_ptr(self.h)
        assert ptr != 0 and self.lib.pdwt_copy(self.h, out.ctypes.data, C.c_void_p(ptr), out.size, 2) == 0
        return out

    def region(self):
        out = np.empty(self.total, dtype=self.spec.dt)
        return int(self.lib.pdwt_get_coeff_region(self.h, out.ctypes.data)), out

    def raw(self):
        """the coefficient region through the device pointer: legal in every state"""
        out = np.empty(self.total, dtype=self.spec.dt)
        ptr = self.lib.pdwt_coeff_ptr(self.h, 0)
        assert ptr != 0 and self.lib.pdwt_copy(self.h, out.ctypes.data, C.c_void_p(ptr), self.total, 2) == 0
        return out

    def split(self, flat):
        return [flat[o:o + n] for o, n in zip(self.offs, self.elems)]

    def _fp(self, a):
        return C.cast(a.ctypes.data, C.POINTER(self.lib.pdwt_real))

    def set_filters(self, which, bank, name):
        s, lib = self.spec, self.lib
        null = C.cast(None, C.POINTER(lib.pdwt_real))
        if s.separable:
            f = [np.ascontiguousarray(t, dtype=s.dt) for t in bank[1:]]
            if which == "fwd":
                return lib.pdwt_set_filters_forward(self.h, name.encode(), s.hlen, self._fp(f[0]), self._fp(f[1]), null, null)
            return lib.pdwt_set_filters_inverse(self.h, self._fp(f[2]), self._fp(f[3]), null, null)
        f = [np.ascontiguousarray(t, dtype=s.dt) for t in (bank[1] if which == "fwd" else bank[2])]  # LL, LH, HL, HH
        if which == "fwd":
            return lib.pdwt_set_filters_forward(self.h, name.encode(), s.hlen, *[self._fp(t) for t in f])
        return lib.pdwt_set_filters_inverse(self.h, *[self._fp(t) for t in f])

    def call(self, op, twin):
        """(return value, data) of one op, as PlanModel.apply returns them"""
        lib, h, s = self.lib, self.h, self.spec
        k, a = op[0], op[1:]
        if self.quiet:
            if k in pm.SLOT_READERS:  # the getters alone (they allocate the workspace where no call has), nothing is copied
                st, th = C.c_void_p(), C.c_void_p()
                getter = lib.pdwt_sparsify_slots if k == "last_sparsify" else lib.pdwt_adaptive_slots
                assert (getter(h, C.byref(th), None) if k == "last_sparsify" else getter(h, C.byref(st), None, None)) == 0
                return 0, None
            if k == "raw_read":  # the pointer getter settles the lazy state: that much of the call stays
                assert lib.pdwt_coeff_ptr(h, 0) != 0
                return 0, None
        if k == "forward":
            return lib.pdwt_forward(h), None
        if k == "inverse":
            return lib.pdwt_inverse(h), None
        if k == "soft":
            return lib.pdwt_soft_threshold(h, *a), None
        if k == "hard":
            return lib.pdwt_hard_threshold(h, *a), None
        if k == "group":
            return lib.pdwt_group_soft_threshold(h, *a), None
        if k == "shrink":
            return lib.pdwt_shrink(h, *a), None
        if k == "linf":
            return lib.pdwt_proj_linf(h, *a), None
        if k in ("norm1", "norm2sq"):
            out = lib.pdwt_real()
            rc = (lib.pdwt_norm1 if k == "norm1" else lib.pdwt_norm2sq)(h, C.byref(out))
            return rc, out.value
        if k in ("norms_async", "soft_norms"):
            from pypwt_amd.wavelets import _read_norms
            rc = lib.pdwt_norms_async(h, None) if k == "norms_async" else lib.pdwt_soft_threshold_norms_async(h, a[0], a[1], a[2], None)
            return rc, (_read_norms(lib, h, None) if rc == 0 and not self.quiet else None)
        if k == "add_dst":
            return lib.pdwt_add_wavelet(h, twin.h, a[0]), None
        if k == "add_src":
            return lib.pdwt_add_wavelet(twin.h, h, a[0]), None
        if k == "get_image":
            out = np.empty((s.batch,) + s.shape, dtype=s.dt)
            return int(lib.pdwt_get_image(h, out.ctypes.data)), out
        if k == "get_image_at":
            out = np.empty(s.shape, dtype=s.dt)
            return int(lib.pdwt_get_image_at(h, out.ctypes.data, a[0])), out
        if k == "get_coeff":
            out = np.full(self.elems[a[0]], 7.0, dtype=s.dt)
            return int(lib.pdwt_get_coeff(h, out.ctypes.data, a[0])), out
        if k == "get_coeff_at":
            out = np.full(self.elems[a[0]] // s.batch, 7.0, dtype=s.dt)
            return int(lib.pdwt_get_coeff_at(h, out.ctypes.data, a[0], a[1])), out
        if k == "get_region":
            return self.region()
        if k == "raw_read":
            return 0, self.raw()
        if k == "set_image":
            img = np.ascontiguousarray(pm.new_image(s, a[0]))
            if a[1]:  # in place: the caller writes the plan's own buffer, the call makes it current
                ptr = lib.pdwt_image_ptr(h)
                assert lib.pdwt_copy(h, C.c_void_p(ptr), img.ctypes.data, img.size, 1) == 0
                return lib.pdwt_set_image(h, C.c_void_p(ptr), 1), None
            return lib.pdwt_set_image(h, img.ctypes.data, 0), None
        if k == "set_coeff":
            shape = (s.batch,) + tuple(s.band_shapes()[a[0]])
            band = np.ascontiguousarray(pm.new_band(s, shape, a[1]))
            if a[2]:
                ptr = lib.pdwt_coeff_ptr(h, a[0])
                assert ptr != 0 and lib.pdwt_copy(h, C.c_void_p(ptr), band.ctypes.data, band.size, 1) == 0
                return lib.pdwt_set_coeff(h, C.c_void_p(ptr), a[0], 1), None
            return lib.pdwt_set_coeff(h, band.ctypes.data, a[0], 0), None
        if k == "clone":
            from pypwt_amd import _lib
            c = _lib.handle_t()
            rc = lib.pdwt_clone(h, C.byref(c))
            return rc, (AbiPlan(s, handle=c, lib=lib) if rc == 0 else None)
        if k == "circshift":
            return lib.pdwt_circshift(h, *a), None
        if k == "filt_fwd":
            return self.set_filters("fwd", s.banks()[a[0]], pm.bank_name(s, a[0])), None
        if k == "filt_inv":
            return self.set_filters("inv", s.banks()[a[0]], ""), None
        watched = not self.quiet
        if k == "band_stats":
            rc = lib.pdwt_band_stats_async(h, None)
            return rc, (self.slots()["band stats"] if rc == 0 and watched else None)
        if k == "estimate_sigma":
            rc = lib.pdwt_estimate_sigma_async(h, a[0], None)
            return rc, (self.slots()["sigma"] if rc == 0 and watched else None)
        if k in ("select", "keep"):
            ks = np.ascontiguousarray(np.atleast_1d(np.asarray(a[0], dtype=np.int64)))
            kp = ks.ctypes.data_as(C.POINTER(C.c_longlong))
            if k == "select":
                rc = lib.pdwt_select_magnitude_async(h, kp, int(ks.size), a[1], None, None)
            else:
                rc = lib.pdwt_keep_largest_async(h, kp, int(ks.size), a[1])
            if rc != 0 or not watched:
                return rc, None
            got = self.slots()
            return rc, (got["sparsify threshold"], got["kept"])
        if k == "threshold_bands":
            T = np.ascontiguousarray(s.table(a[0]))
            opn = 0 if a[1] == "soft" else 1
            if a[2]:
                from test_gpu_adaptive import DevBuf
                self.tables.append(DevBuf(T))
                return lib.pdwt_threshold_bands(h, opn, C.c_void_p(self.tables[-1].__cuda_array_interface__["data"][0]), 1), None
            return lib.pdwt_threshold_bands(h, opn, T.ctypes.data, 0), None
        if k == "denoise":
            method, mode, sigma, skip = a
            sg = None if sigma is None else np.ascontiguousarray(np.atleast_1d(np.asarray(sigma, dtype=np.float64)))
            rc = lib.pdwt_denoise_async(h, 0 if method == "BayesShrink" else 1, 0 if mode == "soft" else 1,
                                        None if sg is None else sg.ctypes.data_as(C.POINTER(C.c_double)), 0 if sg is None else int(sg.size), skip)
            if rc != 0 or not watched:
                return rc, None
            got = self.slots()
            return rc, (got["sigma"], got["table"])
        if k in pm.SLOT_READERS:
            got = self.slots()
            return 0, {"read_band_stats": got["band stats"], "read_sigma": got["sigma"], "last_thresholds": (got["sigma"], got["table"]),
                       "last_sparsify": (got["sparsify threshold"], got["kept"])}[k]
        if k == "take_band":
            # the documented hand-over of device data between two plans: order this plan's stream after the producer's, then pass
            # the producer's own pointer as a device source
            ptr = lib.pdwt_coeff_ptr(twin.h, a[0])  # (settles the producer's lazy state on ITS stream: before the wait)
            assert ptr != 0
            assert lib.pdwt_wait_for_stream(h, C.c_void_p(lib.pdwt_get_stream(twin.h))) == 0, self.last_error()
            return lib.pdwt_set_coeff(h, C.c_void_p(ptr), a[0], 1), None
        raise ValueError(op)


def check_forward(spec, model, got_bands, image, stats):
    """the library's bands against the oracle's (model.bands), then the model adopts them"""
    for num, (g, r) in enumerate(zip(got_bands, model.bands)):
        err = float(np.abs(g.reshape(r.shape).astype(np.float64) - r).max())
        tol = forward_bound(spec, num, r, image)
        stats["forward"] = max(stats["forward"], err / tol)
        assert err <= tol, ("forward: band %d is off by %g, bound %g" % (num, err, tol))
    model.adopt_bands(got_bands)


def check_inverse(spec, model, got_image, bands_before, source, stats):
    want = model.image
    err = float(np.abs(got_image.reshape(want.shape).astype(np.float64) - want).max())
    tol = inverse_bound(spec, bands_before, want)
    stats["inverse"] = max(stats["inverse"], err / tol)
    assert err <= tol, ("inverse: the image is off by %g, bound %g" % (err, tol))
    if source is not None and spec.separable and not spec.custom and spec.prec == "f32":
        # the coefficients are the untouched transform of `source` with the plan's own bank: the round trip, as everywhere
        x = source[0]
        rt = reconstruction_tol(x, spec.wname, spec.levels, ndim=spec.ndim, do_swt=spec.swt)
        assert float(np.abs(got_image.reshape(source.shape)[0] - x).max()) <= rt, "round trip"
    model.adopt_image(got_image)


def new_stats():
    return {"forward": 0.0, "inverse": 0.0, "band_stats": 0.0, "left_out": 0}


def run_ops(spec, ops, seed=0, stats=None, at_end=None, subject=None):
    """Drives the library (C ABI; or `subject`, a stand-in with AbiPlan's interface) and the model with `ops`; returns (calls,
    refused).  `at_end(plan, twin)` runs before the two are closed."""
    stats = stats if stats is not None else new_stats()
    oracle.build()
    image = spec.image(100 + seed)
    if spec.cycle:
        reseed(seed)
    plan = (subject or AbiPlan)(spec, image)
    model = pm.PlanModel(spec, image)
    twin = tmodel = None
    refused = 0
    try:
        assert plan.state() == model.state == pm.INIT
        if spec.custom or not spec.separable:  # the plan's own bank is a custom one: bank 0
            for op in (("filt_fwd", 0), ("filt_inv", 0)):
                assert plan.call(op, None)[0] == model.apply(op)[0] == 0
        # the first forward(), and the twin that add_wavelet needs: a clone
        assert plan.call(("forward",), None)[0] == 0
        model.apply(("forward",), shift=plan.shift())
        stats["shifts"] = [plan.shift()]  # of this run's forwards
        n, flat = plan.region()
        assert n == plan.total == model.region()[1] and plan.offs == model.region()[0]
        check_forward(spec, model, plan.split(flat), model.image, stats)
        rc, twin = plan.call(("clone",), None)
        assert rc == 0
        tmodel = model.clone()
        for i, op in enumerate(ops):
            try:
                refused += _one(spec, plan, model, twin, tmodel, op, stats)
            except AssertionError as e:
                raise AssertionError("%s, call %d %r: %s\n%s" % (spec.name, i, op, e, pm.as_python(spec, seed, ops, i)))
        # what is left at the end, in whatever state the sequence stopped
        flat = plan.raw()
        assert_same_bits(flat, model.flat_region(), "final raw read")
        assert_same_bits(plan.image(), model.image, "final image")
        assert_same_bits(twin.raw(), tmodel.flat_region(), "the twin's final raw read")
        if at_end is not None:
            at_end(plan, twin)
    finally:
        plan.close()
        if twin is not None:
            twin.close()
    return len(ops), refused


def _one(spec, plan, model, twin, tmodel, op, stats):
    k = op[0]
    bands_before, source = model.bands, model.source
    got_rc, got = plan.call(op, twin)
    want_rc, want = model.apply(op, twin=tmodel, shift=plan.shift() if k == "forward" else (0, 0))
    assert got_rc == want_rc, "returned %r, the model %r (%s)" % (got_rc, want_rc, plan.last_error())
    assert plan.state() == model.state, "state %d, the model's %d" % (plan.state(), model.state)
    if pm.refused(op, want_rc):
        if k in ("get_coeff", "get_coeff_at"):
            assert np.all(got == 7.0), "a refused getter wrote its buffer"
        return 1
    if k == "forward":
        stats.setdefault("shifts", []).append(plan.shift())
        n, flat = plan.region()
        assert n == plan.total
        check_forward(spec, model, plan.split(flat), model.image, stats)
        assert_same_bits(flat, model.flat_region(), "the padding after forward()")
    elif k == "inverse":
        check_inverse(spec, model, plan.image(), bands_before, source, stats)
    elif k in ("norm1", "norm2sq"):
        b = norms_bound(plan.total)
        lo, hi = spec.dt(want * (1 - b)), spec.dt(want * (1 + b))  # the getter rounds the fp64 sum to pdwt_real
        assert lo <= got <= hi, "%s = %r, the model's %r" % (k, got, want)
    elif k in ("norms_async", "soft_norms"):
        for g, w in zip(got, want):
            assert abs(g - w) <= norms_bound(plan.total) * w, "%s: %r, the model's %r" % (k, got, want)
    elif k in ("add_dst", "group"):
        n, flat = plan.region()  # nothing is pending after either (both materialise): the read changes nothing
        assert n == plan.total
        assert_close_bands(spec, plan.split(flat), model._flat(), "add" if k == "add_dst" else "group", k)
        model.adopt_bands(plan.split(flat))
    elif k == "add_src":
        n, flat = twin.region()
        assert n == twin.total
        assert_close_bands(spec, twin.split(flat), tmodel._flat(), "add", k)
        tmodel.adopt_bands(twin.split(flat))
    elif k in ("get_image", "get_image_at", "get_coeff", "get_coeff_at", "get_region", "raw_read"):
        assert_same_bits(got, want, k)
    elif k == "clone":
        try:
            assert got.state() == want.state and got.shift() == (want.shift if spec.cycle else got.shift())
            assert_same_bits(got.image(), want.image, "the clone's image")
            assert_same_bits(got.raw(), want.flat_region(), "the clone's coefficients")
            assert got.parent is None and (plan.lib is None or plan.lib.pdwt_image_ptr(got.h) != plan.lib.pdwt_image_ptr(plan.h))
        finally:
            got.close()
    elif k in ("band_stats", "read_band_stats"):
        check_band_stats(model, got, want, stats, k)
    elif k in ("estimate_sigma", "read_sigma"):
        assert_same_bits(got, want, k)
    elif k in ("select", "last_sparsify"):
        assert_same_bits(got[0], want[0], k + ": threshold")
        assert np.array_equal(got[1], want[1]), "%s: kept %r, the model's %r" % (k, got[1], want[1])
    elif k == "keep":
        assert_same_bits(got[0], want[0], k + ": threshold")
        assert np.array_equal(got[1], want[1]), "%s: kept %r, the model's %r" % (k, got[1], want[1])
        assert_same_bits(plan.region()[1], model.flat_region(), k)
    elif k in ("threshold_bands", "take_band"):
        assert_same_bits(plan.raw() if k == "take_band" else plan.region()[1], model.flat_region(), k)
    elif k == "denoise":
        # in two steps, as tests/test_gpu_adaptive.py::test_denoise_in_two_steps: the noise levels exact, the table by its rule,
        # then the sweep bit for bit with the DEVICE's table, which the model adopts
        method, mode = op[1], op[2]
        assert_same_bits(got[0], want[0], k + ": sigma")
        shim = Shim(spec=(spec.name,), dtype=spec.dt, nsamples=spec.shape[0] * spec.shape[1], nbands=spec.nbands, batch=spec.batch)
        ref_stats = adaptive_ref.band_stats(bands_before)
        stats["left_out"] = max(stats["left_out"], left_out_pairs(spec.dt, bands_before, want[0], method, ref_stats))
        check_table(shim, bands_before, want[0], got[1], method, ref_stats)
        model.adopt_table(bands_before, got[1], mode)
        assert_same_bits(plan.region()[1], model.flat_region(), k)
    elif k == "last_thresholds":
        assert_same_bits(got[0], want[0], k + ": sigma")
        assert_same_bits(got[1], want[1], k + ": table")
    return 0


class Shim(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def check_band_stats(model, got, want, stats, what):
    """every entry within 2 n 2^-53 relative, n the swept (padded) length of its band: test_gpu_adaptive.py::test_band_stats"""
    assert got.shape == want.shape and got.dtype == np.float64
    for b, band in enumerate(model.bands):
        bound = 2.0 * swept(band) * U53
        err = np.abs(got[b] - want[b])
        if err.any():
            stats["band_stats"] = max(stats["band_stats"], float((err / (bound * np.maximum(want[b], 1e-300))).max()))
        assert np.all(err <= bound * want[b]), "%s: band %d is %r, the model's %r" % (what, b, got[b], want[b])


def reseed(seed):
    """pdwt_forward draws a cycle-spinning plan's shift with libc's rand(): two runs that are to be compared start it alike"""
    C.CDLL(None).srand(1000 + seed)


# --------------------------------------------------------------------------------------------------------------- C1
@pytest.mark.parametrize("spec", pm.PLANS, ids=lambda s: s.name)
def test_c1_random_sequences_through_the_c_abi(spec):
    stats = new_stats()
    watched_and_blind("C1", spec, pm.SEEDS, stats)


@pytest.mark.parametrize("seed", pm.NEW_SEEDS)
@pytest.mark.parametrize("spec", pm.PLANS, ids=lambda s: s.name)
def test_c1_adaptive_sequences_through_the_c_abi(spec, seed):
    """The seeds that also draw the adaptive and K-term calls, the readers of their slots and take_band (plan_model.NEW_KINDS)."""
    watched_and_blind("C1a seed %d" % seed, spec, (seed,), new_stats())


def writes_norms(ops):
    """does a call of `ops` write the norms slot?  norm1, norm2sq and norms_async are legal in every state; soft_norms counts where
    the state machine does not refuse it (after inverse())"""
    sit = pm.Situation()
    for op in ops:
        if op[0] in ("norm1", "norm2sq", "norms_async") or (op[0] == "soft_norms" and not sit.would_refuse(op[0], False)):
            return True
        sit.step(op, False)
    return False


def snapshot(plan, twin, norms=True):
    """Everything a caller can reach, in a fixed order: state and shift, the image and the whole coefficient region (padding
    included) through their device pointers, the same of the twin, the norms slot (`norms`: once a call has written it -- the
    library does not zero it as it does the others), the adaptive and the sparsify slots.  (The slot getters allocate the
    workspace where no call has: both runs of a comparison do the same.)"""
    out = {"state": np.array([plan.state()]), "shift": np.array(plan.shift())}
    out["image"], out["region"] = plan.image_raw(), plan.raw()
    out["twin state"], out["twin image"], out["twin region"] = np.array([twin.state()]), twin.image_raw(), twin.raw()
    if norms:
        out["norms"] = plan.norms_slot()
    out.update(plan.slots())
    return out


def run_blind(spec, ops, seed, wait=False):
    """The same calls on a fresh plan and its clone with NOTHING read back in between -- the reads of the watched run wait for the
    plan's stream after every call (copy_out and pdwt_copy end in hipStreamSynchronize), which hides what a call finds while the
    previous one is still running: the other plan's stream, the radix-select workspace, the one pinned staging buffer, a result
    slot.  What is left are the waits of the calls themselves (the blocking getters and norms, host sources).  `wait`: both
    streams are waited for after every call instead.  Returns the snapshot at the end, and the shifts the forwards drew."""
    image = spec.image(100 + seed)
    if spec.cycle:
        reseed(seed)
    plan = AbiPlan(spec, image)
    twin = None
    try:
        plan.quiet = True
        if spec.custom or not spec.separable:
            for op in (("filt_fwd", 0), ("filt_inv", 0)):
                assert plan.call(op, None)[0] == 0
        assert plan.call(("forward",), None)[0] == 0
        shifts = [plan.shift()]  # (host state: nothing is waited for)
        rc, twin = plan.call(("clone",), None)
        assert rc == 0
        twin.quiet = True
        for op in ops:
            rc, got = plan.call(op, twin)
            if op[0] == "clone" and got is not None:
                got.close()
            if op[0] == "forward":
                shifts.append(plan.shift())
            if wait:
                assert plan.lib.pdwt_synchronize(plan.h) == 0 and plan.lib.pdwt_synchronize(twin.h) == 0
        out = snapshot(plan, twin, writes_norms(ops))
        out["shifts"] = np.array(shifts)
        return out
    finally:
        plan.close()
        if twin is not None:
            twin.close()


def compare_snapshots(a, b, what):
    assert sorted(a) == sorted(b)
    for key in sorted(a):
        if a[key].dtype.kind == "f":
            assert_same_bits(a[key], b[key], "%s: %s" % (what, key))
        else:
            assert np.array_equal(a[key], b[key]), "%s: %s is %r and %r" % (what, key, a[key], b[key])


def watched_and_blind(tag, spec, seeds, stats):
    """Every sequence twice: checked call by call against the model, then with no host wait between the calls -- the same bits
    everywhere a caller can look, the result slots included."""
    calls = refused = 0
    for seed in seeds:
        ops = pm.sequences()[(spec.name, seed)]
        watched = {}
        n, r = run_ops(spec, ops, seed, stats, at_end=lambda p, t: watched.update(snapshot(p, t, writes_norms(ops))))
        watched["shifts"] = np.array(stats["shifts"])
        calls, refused = calls + n, refused + r
        compare_snapshots(run_blind(spec, ops, seed), watched, "%s, seed %d, without reads in between" % (spec.name, seed))
    for k in WORST:
        WORST[k] = max(WORST[k], stats[k])
    assert stats["left_out"] <= 1 and all(stats[k] <= 1.0 for k in WORST)
    print("SEQ %s %-28s calls %d refused %d left-out %d blind = watched | largest seen/bound: forward %.3f inverse %.3f band_stats %.3f" % (
        tag, spec.name, calls, refused, stats["left_out"], stats["forward"], stats["inverse"], stats["band_stats"]))


# The orderings that the state machine's own comments name, on EVERY plan (the random sequences reach them by their coverage
# conditions, on some plan; these do not depend on a seed): a consumed threshold and set_image, forward() dropping a pending one,
# both operands of add_wavelet, the set_coeff(.., 0) re-arm, a pending threshold that survives set_image, clone and the norms
# after a fused inverse, set_coeff of a detail band while the write-back is owed.
CANNED = [
    ("soft", 12.0, 0, 1), ("inverse",), ("set_image", 901, 0), ("get_region",),
    ("forward",), ("soft", 12.0, 0, 0), ("forward",), ("get_coeff", 1), ("inverse",),
    ("forward",), ("soft", 12.0, 0, 1), ("add_src", 0.5), ("raw_read",),
    ("soft", 12.0, 0, 0), ("add_dst", -1.25), ("inverse",), ("set_coeff", 0, 902, 0), ("inverse",),
    ("forward",), ("soft", 12.0, 0, 1), ("set_image", 903, 1), ("inverse",), ("clone",), ("norm1",), ("set_image", 904, 0),
    ("get_coeff_at", 2, 0),
    ("forward",), ("soft", 12.0, 0, 1), ("inverse",), ("set_coeff", 1, 905, 1), ("set_coeff", 0, 906, 0), ("inverse",), ("raw_read",),
    ("forward",), ("soft_norms", 12.0, 0, 1), ("inverse",), ("norms_async",), ("get_image_at", 0), ("set_image", 907, 0), ("norm2sq",),
]


@pytest.mark.parametrize("spec", pm.PLANS, ids=lambda s: s.name)
def test_c1_named_orderings_on_every_plan(spec):
    stats = new_stats()
    watched = {}
    run_ops(spec, CANNED, 9, stats, at_end=lambda p, t: watched.update(snapshot(p, t, writes_norms(CANNED))))
    watched["shifts"] = np.array(stats["shifts"])
    compare_snapshots(run_blind(spec, CANNED, 9), watched, "%s, the named orderings without reads in between" % spec.name)
    for k in WORST:
        WORST[k] = max(WORST[k], stats[k])


def canned_adaptive(spec):
    """The orderings of the adaptive and K-term calls that share the most state inside a plan, independent of any seed."""
    n0, n1 = spec.swept_count(0), spec.swept_count(1)
    per_image = tuple(1.5 + i for i in range(spec.batch))
    return [
        # the slots before any call has written them: zeros
        ("read_band_stats",), ("read_sigma",), ("last_thresholds",), ("last_sparsify",),
        # the recipe on fresh coefficients, both ways
        ("denoise", "BayesShrink", "soft", None, 1), ("last_thresholds",), ("read_band_stats",),
        ("forward",), ("denoise", "VisuShrink", "hard", None, 0), ("read_sigma",),
        # the radix-select workspace between the noise estimate and the K-term operators
        ("forward",), ("estimate_sigma", 1), ("keep", n0 // 4, 0), ("estimate_sigma", 1), ("read_sigma",), ("select", 5, 1), ("estimate_sigma", 0),
        ("last_sparsify",),
        # the pinned staging buffer behind its one event: K, noise levels, K, a table, noise levels, with nothing waiting in between
        ("forward",), ("keep", n1 // 2, 1), ("denoise", "BayesShrink", "soft", pm.GIVEN_SIGMA, 1), ("select", 5, 0), ("threshold_bands", 911, "hard", 0),
        ("denoise", "VisuShrink", "hard", per_image, 0), ("last_sparsify",), ("last_thresholds",), ("norms_async",), ("band_stats",),
        # a host table directly after the device's own, and a device table (the slot keeps the host's)
        ("forward",), ("denoise", "VisuShrink", "soft", None, 1), ("threshold_bands", 912, "soft", 0), ("last_thresholds",),
        ("threshold_bands", 916, "soft", 1), ("last_thresholds",),
        # a pending threshold in front of every family; a consumed one in front of the read-only ones; the refusals
        ("forward",), ("soft", 12.0, 0, 0), ("band_stats",), ("soft", 12.0, 0, 1), ("threshold_bands", 913, "soft", 1), ("soft", 12.0, 0, 0),
        ("keep", n0 - 1, 0), ("soft", 12.0, 0, 0), ("denoise", "VisuShrink", "soft", 2.5, 1), ("soft", 12.0, 0, 1), ("inverse",),
        ("estimate_sigma", 1), ("keep", 7, 0), ("threshold_bands", 914, "soft", 0), ("denoise", "BayesShrink", "soft", None, 1), ("last_sparsify",),
        ("forward",), ("soft", 12.0, 0, 0), ("inverse",), ("select", n0 // 4, 0), ("get_image_at", 0),
        ("forward",), ("soft", 12.0, 0, 1), ("inverse",), ("band_stats",), ("raw_read",),
        # device data handed from the twin: a detail band while the write-back is owed, then band 0, which re-arms the inverse
        ("forward",), ("add_src", 0.5), ("soft", 12.0, 0, 0), ("inverse",), ("take_band", 2), ("take_band", 0), ("inverse",), ("raw_read",),
    ]


# (not on the plan of 2000 images: the per-image references of its eight tables take the host half a minute; the seeded sequences
# have it)
@pytest.mark.parametrize("spec", [p for p in pm.PLANS if p.batch <= 300], ids=lambda s: s.name)
def test_c1_named_adaptive_orderings(spec):
    stats = new_stats()
    ops = canned_adaptive(spec)
    watched = {}
    run_ops(spec, ops, 9, stats, at_end=lambda p, t: watched.update(snapshot(p, t, writes_norms(ops))))
    watched["shifts"] = np.array(stats["shifts"])
    compare_snapshots(run_blind(spec, ops, 9), watched, "%s, the named adaptive orderings without reads in between" % spec.name)
    for k in WORST:
        WORST[k] = max(WORST[k], stats[k])
    assert stats["left_out"] <= 1 and stats["band_stats"] <= 1.0
    print("SEQ C1n %-28s left-out %d | largest seen/bound: band_stats %.3f" % (spec.name, stats["left_out"], stats["band_stats"]))


# plans whose forward keeps the stream busy for longer than the host needs to enqueue the next calls (2^20 samples a plane and
# more), and a small one
SWT_2K, SWT_1K = pm.Spec("swt2-haar-2048x2048-L2", "swt2", "haar", (2048, 2048), 2), pm.Spec("swt2-haar-1024x1024-L2", "swt2", "haar", (1024, 1024), 2)
DWT_2K = pm.Spec("dwt2-db4-2048x2048-L3", "dwt2", "db4", (2048, 2048), 3)
# (plan, sums in a row before each sweep)
OVERTAKEN = [(SWT_2K, 1), (DWT_2K, 1), ([p for p in pm.PLANS if p.name == "swt2-db3-30x44-L2"][0], 1), (SWT_1K, 6), (DWT_2K, 6)]


def overtaking_ops(queued=1):
    """`queued` sums in a row into the twin before each sweep of the plan: the later ones wait on the twin's stream behind the
    earlier ones while the host goes on to the sweep"""
    busy = [("forward",)] * 4
    return busy + [("add_src", 1.0)] * queued + [("shrink", 3.0, 1)] + busy + [("add_src", -1.25)] * queued + \
        [("soft", 40.0, 1, 0), ("add_dst", 0.5), ("linf", 3.0, 1)]


@pytest.mark.parametrize("spec,queued", OVERTAKEN, ids=lambda v: v.name if isinstance(v, pm.Spec) else "sums%d" % v)
def test_add_wavelet_holds_the_sources_later_work_until_it_has_read(spec, queued):
    """`twin.add_wavelet(plan)` and then, with no host wait, a sweep of `plan` -- the README's FISTA loop has this shape.  The sum
    runs on the twin's stream; pdwt_add_wavelet waited ON THE HOST for the plan's stream and ordered nothing after the sum, so
    the sweep, on the plan's own stream, could overtake the sum's read and the twin received coefficients that were swept in
    part.  pdwt_add_wavelet now orders both ways with events, as pdwt_volume_add_wavelet does: the sum after what the source's
    stream holds, the source's stream after the sum.  Four forwards are queued first, so that the sum (which waits for them) and
    the sweep behind them become ready together; the sweeps change every coefficient they reach (do_app = 1: nothing is deferred).
    The run without waits must leave the bits of the run that waits for both streams after every call.
    Seen on the library before the fix (MI355X, two runs each): with one sum before each sweep the two runs differed on the
    2048 x 2048 stationary plan in one run of two (111 values of the plan's region, 256 of the twin's) and on no smaller or decimated
    plan -- the sum starts first and the sweep rarely catches up with it.  With six sums in a row the later ones wait on the
    twin's stream behind the earlier ones while the sweep starts at once: every run differed on the stationary plans from
    1024 x 1024 on (all 7340032 values of the twin), none on the decimated ones, whose sums are a seventh as long.
    So `swt2-haar-1024x1024-L2-sums6` is the case that pins the fix: it fails on the library before it every time
    (profiles/plan_sequences.txt has that run).  The `sums1` cases are the sequence as first stated; they pass before the fix
    in most runs and guard the ordering from the other side: two event waits must not change a result either."""
    ops = overtaking_ops(queued)
    waited, blind = run_blind(spec, ops, 7, wait=True), run_blind(spec, ops, 7)
    compare_snapshots(blind, waited, "without a wait in between")


def test_norms_after_a_fused_inverse_see_the_thresholded_details():
    """Found by seed 2 of the first plan: soft_threshold (deferred), inverse (applies it on the fly), then norm2sq summed the
    stored, UN-thresholded details (135184144 where the eager semantics give 99091334): the value of the objective of an ISTA
    step depended on whether the plan defers.  The norms now write a consumed threshold back first, like every other reader."""
    spec = pm.PLANS[0]
    run_ops(spec, [("soft", 12.0, 0, 0), ("inverse",), ("inverse",), ("get_coeff_at", 2, 0), ("norm2sq",), ("raw_read",),
                   ("forward",), ("soft", 12.0, 0, 1), ("inverse",), ("norm1",), ("set_coeff", 0, 7, 0), ("inverse",),
                   ("forward",), ("soft_norms", 12.0, 0, 0), ("inverse",), ("norms_async",), ("clone",)])


def _flat_list(coeffs):
    return [coeffs[0]] + [b for lvl in coeffs[1:] for b in (lvl if isinstance(lvl, list) else [lvl])]


def _class_params():
    out = []
    for spec in pm.PLANS:
        out.append(pytest.param(spec, "ctypes", id=spec.name + "-ctypes"))
        if spec.prec == "f32" and not spec.bound:  # the compiled class is float32 and keeps its handle to itself
            out.append(pytest.param(spec, "cython", id=spec.name + "-cython"))
    return out


@pytest.fixture(scope="module")
def W():
    oracle.build()
    from pypwt_amd import Wavelets
    return Wavelets


@pytest.mark.parametrize("spec,binding", _class_params())
def test_c1_random_sequence_through_the_python_class(W, spec, binding):
    """The reference's methods only (plan_model.REFERENCE_KINDS), on one image where the table's plan is a batch: the class has no
    batch.  The class returns nothing from a refused call, so data and exceptions are compared, not status codes; `coeffs` must keep
    handing out the SAME arrays with the current values (test_gpu_ops.py::test_coeffs_are_cached_arrays)."""
    class_sequence(W, spec, binding, pm.CLASS_SEED)


@pytest.mark.parametrize("spec,binding", _class_params())
def test_c1_adaptive_sequence_through_the_python_class(W, spec, binding):
    """... and with the adaptive and K-term methods of both classes (plan_model.CLASS_KINDS; wavelets.py:158-295 and their
    compiled twins): what a method leaves on the device is read through the class's own reader."""
    class_sequence(W, spec, binding, pm.CLASS_SEED_2)


def class_sequence(W, spec, binding, seed):
    if binding == "cython":
        import pycudwt
        assert pycudwt.binding == "cython", "the compiled binding was not built"
        cls = pycudwt.Wavelets
    else:
        from pypwt_amd import Wavelets64
        cls = Wavelets64 if spec.prec == "f64" else W
    one = spec.single()
    ops = pm.sequences()[(spec.name, seed)]
    stats = new_stats()
    image = one.image(100 + seed)

    def host(x):
        return x[0, 0] if one.shape[0] == 1 else x[0]

    def make(img):
        w = cls(host(img), one.wname, one.levels, do_separable=one.separable, do_cycle_spinning=one.cycle, do_swt=one.swt, ndim=one.ndim)
        assert w.levels == one.levels
        return w

    def filters(w, m, bank):
        b = one.banks()[bank]
        name = pm.bank_name(one, bank)
        if one.separable:
            w.set_wavelets_filters(name, b[1], b[2], b[3], b[4])
        else:  # (name, LL, HH, i_LL, i_HH, LH, HL, i_LH, i_HL)
            f, i = b[1], b[2]
            w.set_wavelets_filters(name, f[0], f[3], i[0], i[3], LH=f[1], HL=f[2], i_LH=i[1], i_HL=i[2])
        m.set_filters_forward(b, name)
        m.set_filters_inverse(b)

    w, twin = make(image), make(image)
    model, tmodel = pm.PlanModel(one, image), pm.PlanModel(one, image)
    parent = None
    if one.bound:
        from pypwt_amd import _lib
        lib = _lib.load()
        parent = W(np.zeros((128, 128), dtype=np.float32), "db2", 1)
        assert lib.pdwt_bind_image(w._h, C.c_void_p(lib.pdwt_coeff_ptr(parent._h, 0))) == 0
        w.set_image(host(image))
    if one.custom or not one.separable:
        filters(w, model, 0)
        filters(twin, tmodel, 0)
    cached = None
    for pw, pmod in ((w, model), (twin, tmodel)):
        pw.forward()
        pmod.forward(shift=pw.current_shift)
        co = pw.coeffs
        check_forward(one, pmod, _flat_list(co), pmod.image, stats)
        if pw is w:
            cached = co
    refused = 0
    for i, op in enumerate(ops):
        k, a = op[0], op[1:]
        try:
            bands_before, source = model.bands, model.source
            if k in ("filt_fwd", "filt_inv"):
                filters(w, model, a[0])
                continue
            want_rc, want = model.apply(op, twin=tmodel, shift=(0, 0))
            no = pm.refused(op, want_rc)
            refused += no
            if k == "forward":
                w.forward()
                model.image = model.input  # (again, with the shift the library drew)
                model.forward(shift=w.current_shift)
                co = w.coeffs
                assert co is cached and all(x is y for x, y in zip(_flat_list(co), _flat_list(cached))), "coeffs: new arrays"
                check_forward(one, model, _flat_list(co), model.image, stats)
            elif k == "inverse":
                w.inverse()
                if not no:
                    check_inverse(one, model, w.image[None], bands_before, source, stats)
            elif k == "soft":
                w.soft_threshold(*a)
            elif k == "hard":
                w.hard_threshold(*a)
            elif k == "shrink":
                w.shrink(*a)
            elif k in ("norm1", "norm2sq"):
                got = getattr(w, k)()
                b = norms_bound(model.region()[1])
                assert one.dt(want * (1 - b)) <= got <= one.dt(want * (1 + b)), (got, want)
            elif k == "add_dst":
                assert w.add_wavelet(twin, a[0]) == want_rc
                if not no:
                    got = _flat_list(w.coeffs)
                    assert_close_bands(one, got, model._flat(), "add", k)
                    model.adopt_bands(got)
            elif k == "add_src":
                assert twin.add_wavelet(w, a[0]) == want_rc
                if not no:
                    got = _flat_list(twin.coeffs)
                    assert_close_bands(one, got, tmodel._flat(), "add", k)
                    tmodel.adopt_bands(got)
            elif k == "get_image":
                assert_same_bits(w.image, want, k)
            elif k == "get_coeff":
                if no:
                    with pytest.raises(RuntimeError):
                        w.coeff_only(a[0])
                else:
                    got = w.coeff_only(a[0])
                    assert got is _flat_list(cached)[a[0]], "coeff_only: a new array"
                    assert_same_bits(got, want, k)
            elif k == "get_region":
                if no:
                    with pytest.raises(RuntimeError):
                        w.coeffs
                else:
                    co = w.coeffs
                    assert co is cached
                    for num, g in enumerate(_flat_list(co)):
                        assert_same_bits(g, model.bands[num], "coeffs[%d]" % num)
            elif k == "set_image":
                w.set_image(pm.new_image(one, a[0])[0])  # (Nr, Nc), also for one signal (src/pypwt.pyx: set_image)
            elif k == "set_coeff":
                w.set_coeff(pm.new_band(one, model.bands[a[0]].shape, a[1])[0], a[0])
            elif k in ("band_stats", "read_band_stats"):
                if k == "band_stats":
                    w.band_stats()
                check_band_stats(model, w.read_band_stats(), want, stats, k)
            elif k in ("estimate_sigma", "read_sigma"):
                if k == "estimate_sigma":
                    w.estimate_sigma(skip_zeros=bool(a[0]))
                assert_same_bits(w.read_sigma(), want, k)
            elif k in ("select", "keep", "last_sparsify"):
                if k == "select":
                    w.select_magnitude(k=a[0], do_threshold_appcoeffs=a[1])
                elif k == "keep":
                    w.keep_largest(k=a[0], do_threshold_appcoeffs=a[1])  # after inverse(): a warning, nothing done
                got = w.last_sparsify()
                want = model.sparsify_slot
                assert_same_bits(got[0], want[0], k + ": threshold")
                assert np.array_equal(got[1], want[1]), "%s: kept %r, the model's %r" % (k, got[1], want[1])
                if k == "keep" and not no:
                    for num, g in enumerate(_flat_list(w.coeffs)):
                        assert_same_bits(g, model.bands[num], "coeffs[%d] after keep_largest" % num)
            elif k == "threshold_bands":
                T = np.ascontiguousarray(one.table(a[0]).reshape(-1))
                if a[2]:
                    from test_gpu_adaptive import DevBuf
                    w.threshold_bands(DevBuf(T), a[1])
                else:
                    w.threshold_bands(T, a[1])
                if not no:
                    for num, g in enumerate(_flat_list(w.coeffs)):
                        assert_same_bits(g, model.bands[num], "coeffs[%d] after threshold_bands" % num)
            elif k in ("denoise", "last_thresholds"):
                if k == "denoise":
                    w.denoise(method=a[0], sigma=a[2], mode=a[1], skip_zeros=bool(a[3]))
                sg, T = w.last_thresholds()
                assert_same_bits(sg, model.sigma_slot, k + ": sigma")
                if k == "denoise" and not no:
                    shim = Shim(spec=(one.name, binding), dtype=one.dt, nsamples=one.shape[0] * one.shape[1], nbands=one.nbands, batch=1)
                    ref_stats = adaptive_ref.band_stats(bands_before)
                    stats["left_out"] = max(stats["left_out"], left_out_pairs(one.dt, bands_before, model.sigma_slot, a[0], ref_stats))
                    check_table(shim, bands_before, model.sigma_slot, T.reshape(one.nbands, 1), a[0], ref_stats)
                    model.adopt_table(bands_before, T.reshape(one.nbands, 1), a[1])
                    for num, g in enumerate(_flat_list(w.coeffs)):
                        assert_same_bits(g, model.bands[num], "coeffs[%d] after denoise" % num)
                else:
                    assert_same_bits(T, model.table_slot, k + ": table")
            else:
                raise ValueError(op)
        except AssertionError as e:
            raise AssertionError("%s (%s class), call %d %r: %s\ncalls so far: %r" % (spec.name, binding, i, op, e, ops[:i + 1]))
    print("SEQ C1 %-28s %s class, seed %d: calls %d refused %d left-out %d | largest seen/bound: forward %.3f inverse %.3f band_stats %.3f" % (
        spec.name, binding, seed, len(ops), refused, stats["left_out"], stats["forward"], stats["inverse"], stats["band_stats"]))
    for k in WORST:
        WORST[k] = max(WORST[k], stats[k])
    assert stats["left_out"] <= 1 and stats["band_stats"] <= 1.0
    del parent


# --------------------------------------------------------------------------------------------------------------- C2
SOFT_FAMILIES = {"swt2_inv_stream+soft", "swt2_inv_split+soft", "swt2_inv_level+soft", "swt2_inv_tail+soft", "swt2_inv_fused+soft"}
FUSING_CASES = [c for c in DISPATCH_CASES if c[0] == "swt2"] + [
    # batch 3 of one mid-size plan per family
    ("swt2", "haar", (301, 515), 3, 3, "f32"),      # fused groups
    ("swt2", "db2", (514, 1023), 4, 3, "f32"),      # 4-tap fused pairs
    ("swt2", "db4", (512, 512), 3, 3, "f32"),       # one-launch stream levels, 8 taps
    ("swt2", "db10", (250, 1022), 2, 3, "f32"),     # ... 20 taps
    ("swt2", "db3", (30, 44), 2, 3, "f32"),         # level launches (the one-workgroup launch is a batch in the table already)
    ("swt2", "db20", (256, 256), 2, 3, "f32"),      # row + column launches
    ("swt2", "db4", (256, 256), 2, 3, "f64"),
]
BETA_C2 = 12.0


def _names(plan):
    return [n for n, _ in plan.p.kernel_times()]


def _fill(plan):
    kind, w, shape, L, B, prec = plan.case
    if prec == "f64":
        plan.p.set_image(np.stack([oracle.hash_input(shape, 4242, index_offset=b * shape[0] * shape[1]).astype(plan.dt) for b in range(B)]))
    else:
        plan.p.fill_hash(4242, 255.0)


def _image(plan):
    """the image through its device pointer (no getter, no state)"""
    kind, w, shape, L, B, prec = plan.case
    out = np.empty(B * shape[0] * shape[1], dtype=plan.dt)
    ptr = plan.lib.pdwt_image_ptr(plan.h)
    assert ptr != 0 and plan.lib.pdwt_copy(plan.h, out.ctypes.data, C.c_void_p(ptr), out.size, 2) == 0
    return out


@pytest.mark.parametrize("case", FUSING_CASES, ids=lambda c: "%s-%s-%dx%d-L%d-b%d-%s" % (c[0], c[1], c[2][0], c[2][1], c[3], c[4], c[5]))
def test_c2_fused_threshold_equals_the_eager_one_bit_for_bit(case):
    oracle.build()
    reached = set()
    for normalize in (0, 1):
        E, F = Plan(case), Plan(case)
        try:
            for p in (E, F):
                _fill(p)
                p.p.forward()
            before = E.download()  # nothing pending yet
            assert ops_ref.same_bits(before, F.download()), "two plans, one image, different coefficients"
            for p in (E, F):
                assert p.lib.pdwt_soft_threshold(p.h, BETA_C2, 0, normalize) == 0
            n1 = E.lib.pdwt_real()
            assert E.lib.pdwt_norm1(E.h, C.byref(n1)) == 0  # E: the threshold is applied to the stored details now
            for p in (E, F):
                p.p.enable_kernel_timing(True)
                p.p.reset_kernel_times()
                p.p.inverse()
            ne, nf = [n for n in _names(E) if n.startswith("swt2_inv")], [n for n in _names(F) if n.startswith("swt2_inv")]
            assert nf and all(n.endswith("+soft") for n in nf), (case, nf)
            assert ne == [n[:-len("+soft")] for n in nf], (case, ne, nf)
            reached |= set(nf)
            img_e, img_f = _image(E), _image(F)
            assert ops_ref.same_bits(img_e, img_f), "%s normalize %d: fused and eager images differ in %d values, by up to %g" % (
                case, normalize, int((img_e != img_f).sum()), float(np.abs(img_e - img_f).max()))
            # re-arm both, read every band of both raw: the write-back F owed equals what E stored, and both the reference operator
            a0 = np.ascontiguousarray(E.bands(before)[0])
            for p in (E, F):
                assert p.lib.pdwt_set_coeff(p.h, a0.ctypes.data, 0, 0) == 0
            flat_e, flat_f = E.download(after_inverse=True), F.download(after_inverse=True)
            assert ops_ref.same_bits(flat_e, flat_f), "the coefficients after the write-back differ from the eager plan's"
            want = ops_ref.threshold(E.bands(before), E.L, 2, "soft", BETA_C2, 0, normalize)
            for k, (g, r) in enumerate(zip(E.bands(flat_e), want)):
                assert ops_ref.same_bits(g, r), (case, normalize, "band %d is not soft(band read before the threshold)" % k)
            E.check_padding(flat_e, "after the write-back")
            for p in (E, F):
                p.p.reset_kernel_times()
                p.p.inverse()
            assert not any(n.endswith("+soft") for n in _names(F)), "nothing is pending at the second inverse"
            assert ops_ref.same_bits(_image(E), _image(F)), "second inverse"
            assert ops_ref.same_bits(_image(F), img_f), "the second inverse of the same coefficients gives another image"
        finally:
            E.close()
            F.close()
    print("SEQ C2 %s reached %s" % (case, sorted(reached)))


def test_c2_every_fusing_family_is_reached():
    """the five `+soft` launches of plan.cpp all run at the default dispatch on the plans above"""
    union = set()
    for case in FUSING_CASES:
        F = Plan(case)
        try:
            _fill(F)
            F.p.forward()
            assert F.lib.pdwt_soft_threshold(F.h, BETA_C2, 0, 1) == 0
            F.p.enable_kernel_timing(True)
            F.p.reset_kernel_times()
            F.p.inverse()
            union |= {n for n in _names(F) if n.startswith("swt2_inv")}
        finally:
            F.close()
    assert union == SOFT_FAMILIES, (sorted(SOFT_FAMILIES - union), sorted(union - SOFT_FAMILIES))


# --------------------------------------------------------------------------------------------------------------- C3
@pytest.mark.parametrize("case", DISPATCH_CASES, ids=lambda c: "%s-%s-%dx%d-L%d-b%d-%s" % (c[0], "custom" if isinstance(c[1], tuple) else c[1], c[2][0], c[2][1], c[3], c[4], c[5]))
def test_c3_transforms_leave_their_inputs_alone(case):
    """forward() does not write its image (pdwt_bind_image makes it another plan's band 0), inverse() does not write the
    coefficients (plan.hpp:13-16; set_coeff(.., 0) re-arms it), and a plan gives the same bits in round 5 as in round 1."""
    plan = Plan(case)
    try:
        _fill(plan)
        x = _image(plan)
        plan.p.forward()
        assert ops_ref.same_bits(_image(plan), x), "forward() wrote its image"
        co = plan.download(after_inverse=True)  # pdwt_coeff_ptr + pdwt_copy; nothing is pending, so nothing is written
        plan.check_padding(co, "after forward")
        plan.p.inverse()
        co2 = plan.download(after_inverse=True)
        if not ops_ref.same_bits(co, co2):
            bad = [k for k, (a, b) in enumerate(zip(plan.bands(co), plan.bands(co2))) if not ops_ref.same_bits(a, b)]
            raise AssertionError("%s: inverse() wrote the coefficients: bands %s (or their padding) changed" % (case, bad))
        img1 = _image(plan)
        a0 = np.ascontiguousarray(plan.bands(co)[0])
        assert plan.lib.pdwt_set_coeff(plan.h, a0.ctypes.data, 0, 0) == 0
        plan.p.inverse()
        assert ops_ref.same_bits(_image(plan), img1), "the inverse re-armed by set_coeff(.., 0) gives another image"
        for _ in range(5):
            assert plan.lib.pdwt_set_image(plan.h, x.ctypes.data, 0) == 0
            plan.p.forward()
            plan.p.inverse()
        assert ops_ref.same_bits(plan.download(after_inverse=True), co), "round 5: other coefficients than round 1"
        assert ops_ref.same_bits(_image(plan), img1), "round 5: another image than round 1"
    finally:
        plan.close()


def test_report():
    print("SEQ largest seen/bound of the comparisons with a bound: forward %.3f inverse %.3f band_stats %.3f" % (WORST["forward"], WORST["inverse"], WORST["band_stats"]))
