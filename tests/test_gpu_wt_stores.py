"""Write-through whole-line stores (pdwt_set_tuning("wt_stores"): launch_dwt2.hip wt_stores_take, InvCoarse3Args::wt_out) on the
GPU.  The inverse coarse group is the one launch that has them: the level-1 inverse tile and the forward tile lost their A/B
(docs/LAB_NOTEBOOK.md) and store as before, which the counts below also say.

The policy changes how bytes leave a launch, not arithmetic: a plan built under "wt_stores" = 2 (wherever the stores' preconditions
hold) and one built under 0 on the same input must give BITWISE equal coefficient planes and reconstructions, the same launch names
and kernel families, and both must meet the project's bound against the oracle (tests/test_gpu_dispatch.py: coefficients
8 ulps (1 + L) of max(|band|, 255), the reconstruction 2e-6 (1 + L) 255 absolute against oracle.inverse of the plan's own
coefficients, as tests/test_gpu_inv_coarse.py).  The process-wide count of launches that stored write-through ("wt_stores_launches")
moves for the = 2 plan and stays for the = 0 plan.

Cases: whole and partial tiles on both axes with a batch, one level (level launches only: nothing may count) and three (the group
writes the images of the batch); an image whose coefficient rows are not whole 16-B groups (nothing may count in either direction);
the coarse group under a level-1 launch and the group writing the image itself ("inv_coarse3" = 2 brings the group to planes this
small).  haar,
db2, db4 and a random 8-tap bank whose every tap counts (scaled as in tests/test_gpu_inv_coarse.py so that the bound's 255 holds)."""
import ctypes as C

import numpy as np
import pytest

import tap_banks
from inv_coarse_geom import supported
from oracle import oracle

pytestmark = pytest.mark.gpu

# (rows, columns), levels, batch
CASES = [((64, 96), 1, 3), ((64, 96), 3, 3), ((72, 288), 1, 3), ((72, 288), 3, 3), ((40, 76), 1, 1), ((512, 512), 4, 1), ((512, 512), 3, 1)]
FILTERS = ["haar", "db2", "db4", "random8"]


@pytest.fixture(scope="module")
def lib():
    from pypwt_amd import _lib
    return _lib.load()


def _set_filters(plan, filt):
    rp = C.POINTER(C.c_float)
    ptr = [C.cast(t.ctypes.data, rp) for t in filt[1:]]
    null = C.cast(None, rp)
    assert plan._lib.pdwt_set_filters_forward(plan._h, b"custom", filt[0], ptr[0], ptr[1], null, null) == 0
    assert plan._lib.pdwt_set_filters_inverse(plan._h, ptr[2], ptr[3], null, null) == 0


def _plan(lib, mode, B, Nr, Nc, wname, L, img=None, coarse=2):
    from pypwt_amd import BatchedWavelets
    was = lib.pdwt_set_tuning(b"wt_stores", mode)
    was3 = lib.pdwt_set_tuning(b"inv_coarse3", coarse)
    try:
        return BatchedWavelets(B, Nr, Nc, wname, L, img=img)
    finally:
        lib.pdwt_set_tuning(b"inv_coarse3", was3)
        lib.pdwt_set_tuning(b"wt_stores", was)


def _run(lib, mode, x, wname, filt, L):
    """One plan built under "wt_stores" = mode: (launches of the forward, of the inverse, coefficients, reconstruction, levels,
    write-through launches counted during the forward, during the inverse)."""
    B, Nr, Nc = x.shape
    plan = _plan(lib, mode, B, Nr, Nc, wname if filt is None else "db4", L, img=x)
    try:
        if filt is not None:
            _set_filters(plan, filt)
        L = plan.levels
        plan.enable_kernel_timing(True)
        plan.reset_kernel_times()
        lib.pdwt_set_tuning(b"wt_stores_launches", 0)
        plan.forward()
        n_fwd = lib.pdwt_set_tuning(b"wt_stores_launches", 0)
        fwd = list(zip([n for n, _ in plan.kernel_times()], plan.kernel_families()))
        coeffs = [[plan.coeff_at(num, b).copy() for num in range(3 * L + 1)] for b in range(B)]
        plan.reset_kernel_times()
        plan.inverse()
        n_inv = lib.pdwt_set_tuning(b"wt_stores_launches", 0)
        inv = list(zip([n for n, _ in plan.kernel_times()], plan.kernel_families()))
        return fwd, inv, coeffs, np.array(plan.image, copy=True), L, n_fwd, n_inv
    finally:
        plan.cleanup()


@pytest.mark.parametrize("wname", FILTERS)
def test_write_through_plans_equal_plain_plans_bit_for_bit(lib, wname):
    filt = tap_banks.bank(8, 77) if wname == "random8" else None
    for ci, (shape, L, B) in enumerate(CASES):
        x = np.stack([oracle.hash_input(shape, 8800 + ci, index_offset=b * shape[0] * shape[1]) for b in range(B)]).astype(np.float32)
        if filt is not None:  # scale so that the reconstruction the bound speaks of stays within 255
            probe = _plan(lib, 0, 1, shape[0], shape[1], "db4", L)
            L = probe.levels
            probe.cleanup()
            peak = max(float(np.abs(oracle.inverse(oracle.forward(x[b], None, L, filt=filt), shape, None, L, filt=filt)).max()) for b in range(B))
            x *= np.float32(min(1.0, 255.0 / peak))
        on = _run(lib, 2, x, wname, filt, L)
        off = _run(lib, 0, x, wname, filt, L)
        L = on[4]
        assert off[4] == L
        tag = (wname, shape, L, B)
        # the same launches, the same families
        assert on[0] == off[0] and on[1] == off[1], (tag, on[:2], off[:2])
        # bitwise equal coefficients and reconstruction
        for b in range(B):
            for num in range(3 * L + 1):
                assert np.array_equal(on[2][b][num].view(np.uint32), off[2][b][num].view(np.uint32)), (tag, "coefficients", b, num)
        assert np.array_equal(on[3].view(np.uint32), off[3].view(np.uint32)), (tag, "reconstruction")
        # both meet the project's bound against the oracle
        cbound = 8 * 1.2e-7 * (1 + L)
        rbound = 2e-6 * (1 + L) * 255.0
        for name, (_, _, coeffs, rec, _, _, _) in (("on", on), ("off", off)):
            for b in range(B):
                ref = oracle.forward(x[b], None if filt else wname, L, filt=filt)
                cerr = max(float(np.abs(g.reshape(r.shape) - r).max()) / max(float(np.abs(r).max()), 255.0) for g, r in zip(coeffs[b], ref))
                want = oracle.inverse(coeffs[b], shape, None if filt else wname, L, filt=filt)
                rerr = float(np.abs(rec[b].reshape(want.shape) - want).max())
                print("wt_stores %s %s L%d B%d %s: cerr %.3g bound %.3g | rerr %.3g bound %.3g | counted fwd %d inv %d"
                      % (wname, shape, L, B, name, cerr, cbound, rerr, rbound, on[5] if name == "on" else off[5], on[6] if name == "on" else off[6]))
                assert cerr <= cbound, (tag, name, b, cerr, cbound)
                assert rerr <= rbound, (tag, name, b, rerr, rbound)
        # the counter: the forward has no write-through path; of the inverse's launches the coarse group took it (its output rows
        # are whole 16-B groups wherever it applies), the level launches did not; the = 0 plan never
        assert off[5] == 0 and off[6] == 0, (tag, off[5:])
        assert on[5] == 0, (tag, "the forward counted", on[5])
        hlen = filt[0] if filt else oracle.filters(wname)[0]
        group = L >= 3 and supported(hlen, (shape[0] >> (L - 3), shape[1] >> (L - 3)))  # the coarse group serves levels L-2 .. L
        assert on[6] == (1 if group else 0), (tag, on[1], on[6])
        if shape == (512, 512) or L == 3:
            assert group and on[1][0] == ("dwt2_inv_pyr3", "") and on[6] == 1, (tag, on[1], on[6])
        if shape == (40, 76):
            assert on[1] == [("dwt2_inv_level", "tile")] and on[6] == 0, (tag, on[1], on[6])


def test_default_rule(lib):
    """"wt_stores" = 1: one 4096^2 image takes the policy in its coarse group; sixteen images and a 1024^2 image do not
    (tuning_gfx950.inc: plans of at most 2^wt_stores_max_log2 = 2^24 samples, launches that write at least 2^wt_stores_min_log2 = 2^22)."""
    assert lib.pdwt_set_tuning(b"wt_stores", 1) == 1, "the key's initial value is 1: the size rule"

    def counted(B, n, L):
        plan = _plan(lib, 1, B, n, n, "db4", L, coarse=1)
        try:
            plan.forward()
            lib.pdwt_set_tuning(b"wt_stores_launches", 0)
            plan.inverse()
            return lib.pdwt_set_tuning(b"wt_stores_launches", 0)
        finally:
            plan.cleanup()

    assert counted(1, 4096, 4) == 1
    assert counted(16, 4096, 4) == 0
    assert counted(1, 1024, 3) == 0


def test_a_clone_keeps_the_value_of_its_source(lib):
    src = _plan(lib, 2, 1, 64, 96, "db4", 3, img=oracle.hash_input((64, 96), 8899)[None])  # inv: the coarse group alone
    try:
        h = C.c_void_p()
        assert lib.pdwt_set_tuning(b"wt_stores", 0) == 1  # the process-wide value while the clone is made
        try:
            assert lib.pdwt_clone(src._h, C.byref(h)) == 0
        finally:
            lib.pdwt_set_tuning(b"wt_stores", 1)
        try:
            assert lib.pdwt_forward(h) == 0
            lib.pdwt_set_tuning(b"wt_stores_launches", 0)
            assert lib.pdwt_inverse(h) == 0 and lib.pdwt_synchronize(h) == 0
            assert lib.pdwt_set_tuning(b"wt_stores_launches", 0) == 1
        finally:
            lib.pdwt_destroy(h)
    finally:
        src.cleanup()
