"""The inverse of the three coarsest levels in one launch (pypwt_amd/csrc/dwt2_inv_coarse_kernels.hpp) on the GPU.

The default dispatch sends only large planes there (more than 2^20 and at most 2^22 samples: the 2048^2 plane of one 4096^2
image); pdwt_set_tuning("inv_coarse3", 2) takes the group wherever the kernel applies, which is how these tests reach it on planes
small enough to be cheap: smaller than any tile (declined: the launch list must be the one of "inv_coarse3" = 0), one tile with
regions that wrap on both axes, partial tiles on both axes, a batch, the group under a level-1 launch (the headline's schedule in
small) and the group writing the image itself.  haar, db2, db3, db4 and a random 8-tap bank whose every tap counts.

Every reconstruction is compared with oracle.inverse of the SAME coefficients (read back from the plan after its forward) at the
project's bound, 2e-6 (1 + L) 255 absolute (tests/test_gpu_dispatch.py); the "inv_coarse3" = 0 plan on the same input meets the same
bound.  The bound speaks of samples of magnitude 255: the random bank is no perfect-reconstruction pair, so its input is scaled (on
the CPU, by the oracle's own round trip, before anything runs on the GPU) so that the reconstruction stays within 255."""
import ctypes as C

import numpy as np
import pytest

import tap_banks
from inv_coarse_geom import supported
from oracle import oracle

pytestmark = pytest.mark.gpu

# (rows, columns), levels, batch
CASES = [((32, 32), 3, 1), ((64, 96), 3, 1), ((32, 256), 3, 1), ((256, 32), 3, 1), ((72, 288), 3, 3), ((512, 512), 4, 1),
         ((512, 512), 3, 1)]
FILTERS = ["haar", "db2", "db3", "db4", "random8"]


def _bank(name):
    return tap_banks.bank(8, 77) if name == "random8" else None


def _set_filters(plan, filt):
    rp = C.POINTER(C.c_float)
    ptr = [C.cast(t.ctypes.data, rp) for t in filt[1:]]
    null = C.cast(None, rp)
    assert plan._lib.pdwt_set_filters_forward(plan._h, b"custom", filt[0], ptr[0], ptr[1], null, null) == 0
    assert plan._lib.pdwt_set_filters_inverse(plan._h, ptr[2], ptr[3], null, null) == 0


def _run(lib, mode, x, wname, filt, L):
    """One plan built under "inv_coarse3" = mode: (inverse schedule, inverse launch names, coefficients, reconstruction)."""
    from pypwt_amd import BatchedWavelets
    B, Nr, Nc = x.shape
    was = lib.pdwt_set_tuning(b"inv_coarse3", mode)
    try:
        plan = BatchedWavelets(B, Nr, Nc, wname if filt is None else "db4", L, img=x)
    finally:
        lib.pdwt_set_tuning(b"inv_coarse3", was)
    try:
        if filt is not None:
            _set_filters(plan, filt)  # (rebuilds the launch lists from the plan's own value of the key)
        L = plan.levels  # (a 32 x 32 image holds two levels of a 6- or 8-tap filter: the library lowers the count, as the reference does)
        plan.forward()
        coeffs = [[plan.coeff_at(num, b) for num in range(3 * L + 1)] for b in range(B)]
        plan.enable_kernel_timing(True)
        plan.reset_kernel_times()
        plan.inverse()
        names = [n for n, _ in plan.kernel_times()]
        fams = plan.kernel_families()
        sched = [ln for ln in plan.schedule().splitlines() if ln.startswith("inv:")][0]
        return sched, list(zip(names, fams)), coeffs, plan.image, L
    finally:
        plan.cleanup()


@pytest.fixture(scope="module")
def lib():
    from pypwt_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("wname", FILTERS)
def test_inv_coarse3_matches_the_oracle_where_taken_and_where_declined(lib, wname):
    filt = _bank(wname)
    hlen = filt[0] if filt else oracle.filters(wname)[0]
    for ci, (shape, L, B) in enumerate(CASES):
        x = np.stack([oracle.hash_input(shape, 7700 + ci, index_offset=b * shape[0] * shape[1]) for b in range(B)]).astype(np.float32)
        if filt is not None:  # scale so that the reconstruction the bound speaks of stays within 255 (module docstring)
            from pypwt_amd import BatchedWavelets
            probe = BatchedWavelets(1, shape[0], shape[1], "db4", L)
            L = probe.levels  # (the count the library grants an 8-tap filter on this size)
            probe.cleanup()
            peak =max(float(np.abs(oracle.inverse(oracle.forward(x[b], None, L, filt=filt), shape, None, L, filt=filt)).max()) for b in range(B))
            x *= np.float32(min(1.0, 255.0 / peak))
        on = _run(lib, 2, x, wname, filt, L)
        off = _run(lib, 0, x, wname, filt, L)
        L = on[4]  # the levels the plan has
        assert off[4] == L
        group = (shape[0] >> max(L - 3, 0), shape[1] >> max(L - 3, 0))  # the plane the group writes
        want_taken = L >= 3 and supported(hlen, group)
        bound = 2e-6 * (1 + L) * 255.0
        for tag, (sched, launches, coeffs, rec, _) in (("on", on), ("off", off)):
            for b in range(B):
                want = oracle.inverse(coeffs[b], shape, None if filt else wname, L, filt=filt)
                err = float(np.abs(rec[b] - want).max())
                print("inv_coarse3 %s %s L%d B%d %s: %s | err %.3g bound %.3g" % (wname, shape, L, B, tag, sched, err, bound))
                assert err <= bound, (wname, shape, L, tag, b, err, bound)
        names = [n for n, _ in on[1]]
        if want_taken:
            assert ("dwt2_inv_pyr3", "") in on[1], (wname, shape, on[1])
            assert on[0].split() == ["inv:", "PYR3[%d-%d]" % (L - 2, L)] + ["LEVEL[%d]" % l for l in range(L - 3, 0, -1)], (wname, shape, on[0])
            assert names == ["dwt2_inv_pyr3"] + ["dwt2_inv_level"] * (L - 3), (wname, shape, names)
        else:
            assert on[0] == off[0] and on[1] == off[1], (wname, shape, "declined, yet not the launch list of inv_coarse3 = 0", on[:2], off[:2])
        if shape == (32, 32):
            assert not want_taken
        if shape == (512, 512):
            assert want_taken
            if L == 4:  # today's list has no three-level launch here: the name can only come from the new kernel
                assert "dwt2_inv_pyr3" not in [n for n, _ in off[1]], off[1]


def test_default_schedules(lib):
    """The default rule takes the headline plan's coarse levels and nothing else that the benchmark measures."""
    from pypwt_amd import BatchedWavelets

    def sched(mode, B, n, L):
        was = lib.pdwt_set_tuning(b"inv_coarse3", mode)
        try:
            plan = BatchedWavelets(B, n, n, "db4", L)
        finally:
            lib.pdwt_set_tuning(b"inv_coarse3", was)
        try:
            return plan.schedule()
        finally:
            plan.cleanup()

    assert lib.pdwt_set_tuning(b"inv_coarse3", 1) == 1, "the key's initial value is 1: the size rule"
    head = sched(1, 1, 4096, 4)
    assert [ln for ln in head.splitlines() if ln.startswith("inv:")][0].split() == ["inv:", "PYR3[2-4]", "LEVEL[1]"], head
    assert [ln for ln in head.splitlines() if ln.startswith("fwd:")] == [ln for ln in sched(0, 1, 4096, 4).splitlines() if ln.startswith("fwd:")]
    assert sched(1, 16, 4096, 4) == sched(0, 16, 4096, 4)
    assert sched(1, 1, 1024, 3) == sched(0, 1, 1024, 3)
