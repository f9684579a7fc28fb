"""Tap-resolved GPU parity: random filter banks whose every tap counts (tests/tap_banks.py) through every fp32 kernel family that takes
filters longer than 20 taps, at the tolerance the reference itself sets.

The family modules compare the built-in wavelets on a 0..255 image at an absolute 2e-6 (1 + L) max(|band|, 255); db11-db20, sym14-sym20,
coif4 and coif5 have 1-9 taps of dec_lo below what that sees (tests/test_tap_banks_cpu.py pins it), exactly where the long-filter
kernels keep one template instantiation per length with histories, warm-ups and hlen / 2 parities of their own.  Here every tap is at
least 0.079, the four filters are independent, and a kernel is compared with the oracle's fp64-accumulating result at K x the fp32
oracle's own distance from it (tap_banks.K = 4; the largest measured ratios are in profiles/taps_parity.txt), floored at one ulp.  The
inverse is tested on its own: it starts from the oracle's coefficients (set_coeff), not from the forward kernel's.

Every case forces its family the way the family's own module does (pdwt_set_tuning keys 100 + n, PDWT_NO_PYRAMID, PDWT_NO_TAIL ...,
restored afterwards), creates the plan with a built-in wavelet of the same length (so the level count is that length's), replaces the
bank (pdwt_set_filters_forward rebuilds the schedule from hlen), and asserts through kernel_times() / kernel_families() that the
intended (launch name, family) ran in each direction: a silent fall-back fails.  Shapes are the ragged ones of the family modules,
one whose axes are shorter than the filter (it wraps more than once), one batch of three (odd sizes where the family takes them;
images 0 and B - 1 are checked); SWT families run levels 1-3 (dilations 1, 2, 4).

Not reachable beyond 20 taps, hence absent: the tile pyramids dwt2_*_pyr2 / pyr3 (at most 16 taps), strip2 and the wave kernels (8),
the register ring (20), dwt1_*_reg (20), the fused SWT groups (2 and 4 taps); the level-count rule of dwt2_*_tail (a long filter
clamps a small plane to one level) -- its batch mode is here.  The two-launch decimated levels (launch_dwt2_split.hip, 10-40 taps) are
an experiment that lives in the test-only library, not in the product: tests/test_gpu_parity.py::test_dwt_two_launch_levels keeps
them covered, they are not repeated here.  Odd lengths (21, 39) run where a family has an any-length instantiation: the decimated
generic kernels, dwt1 and swt1 levels, the SWT tiles.

Out of scope:
  * decimated 2-tap banks: the oracle restates the reference's hard-coded Haar butterflies there, a custom 2-tap bank has no oracle
    (and both Haar taps are 0.707);
  * the families of at most 20 taps beyond one length each (SHORT below: wave, ring, pyr3, fused 4-tap SWT, reg1d): their built-in
    taps are all visible to the usual tolerance, the single case guards this module's helper.  strip2 has none: it starts at 2^26
    samples per launch;
  * the fp64 library: its tolerances (1e-12 relative) sit far below a 2e-10 tap times 255;
  * non-separable banks: they have a random-bank test at their sizes already."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle
import tap_banks

pytestmark = pytest.mark.gpu

RATIOS = {}  # (family, direction) -> largest err / noise seen


@contextlib.contextmanager
def forced(keys=(), env=()):
    """pdwt_set_tuning keys and environment variables (read when a plan is built) for one case; restored afterwards."""
    from pypwt_amd import _lib
    lib = _lib.load()
    prev, had = [], []
    try:
        for k, v in keys:
            was = lib.pdwt_set_tuning(k.encode(), v)
            assert was >= 0, k
            prev.append((k, was))
        for name in env:
            had.append((name, os.environ.get(name)))
            os.environ[name] = "1"
        yield
    finally:
        for name, was in had:
            if was is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = was
        for k, was in reversed(prev):
            lib.pdwt_set_tuning(k.encode(), was)


def base_wavelet(n):
    """A built-in wavelet of n taps (n + 1 for an odd n: there is none): the plan's level count is that length's."""
    table = oracle.filter_table()["filters"]
    want = n + (n & 1)
    for name in ("db%d" % (want // 2), "sym%d" % (want // 2)):
        if name in table and table[name]["hlen"] == want:
            return name
    return sorted(k for k, e in table.items() if e["hlen"] == want)[0]


def _set_bank(plan, filt):
    rp = C.POINTER(C.c_float)
    ptr = [C.cast(t.ctypes.data, rp) for t in filt[1:]]
    null = C.cast(None, rp)
    assert plan._lib.pdwt_set_filters_forward(plan._h, b"taps", filt[0], ptr[0], ptr[1], null, null) == 0
    assert plan._lib.pdwt_set_filters_inverse(plan._h, ptr[2], ptr[3], null, null) == 0


def _launches(plan):
    pairs = list(zip([n for n, _ in plan.kernel_times()], plan.kernel_families()))
    plan.reset_kernel_times()
    return pairs


def _note(family, direction, err, noise):
    key = (family, direction)
    RATIOS[key] = max(RATIOS.get(key, 0.0), _ratio(err, noise))


def _served(launches, want):
    """`want` is one (launch name, family): EVERY launch of the direction must be it (a level that fell back to another family
    fails); or the exact list of launches, where a case names the level another family serves."""
    return launches == list(want) if isinstance(want, list) else bool(launches) and set(launches) == {want}


def _ratio(err, noise):
    return err / noise if noise > 0 else (0.0 if err == 0 else float("inf"))


def run_case(family, kind, n, shape, levels, batch, want_fwd, want_inv, seed=0):
    """One plan: forward against the f64acc oracle, then the oracle's coefficients through the inverse; every launch of a direction
    must be want_fwd / want_inv (see _served).  Returns the clamped level count."""
    from pypwt_amd import BatchedWavelets
    ndim, swt = (2 if kind in ("dwt2", "swt2") else 1), (1 if kind.startswith("swt") else 0)
    filt = tap_banks.bank(n, 1000 + seed)
    x = np.stack([oracle.hash_input(shape, 7700 + 31 * n + seed + b) for b in range(batch)])
    plan = BatchedWavelets(batch, shape[0], shape[1], base_wavelet(n), levels, do_swt=swt, ndim=ndim, img=x)
    try:
        _set_bank(plan, filt)
        L = plan.levels
        plan.enable_kernel_timing(True)
        plan.reset_kernel_times()
        plan.forward()
        fwd = _launches(plan)
        tag = (family, kind, n, shape, L, batch)
        print("taps %-10s n=%2d %s L%d B%d fwd launches %s" % (family, n, shape, L, batch, fwd))
        assert _served(fwd, want_fwd), (tag, "forward ran", fwd, "wanted", want_fwd)
        checked = sorted({0, batch - 1})
        refs = {}
        for b in checked:
            refs[b], tols = tap_banks.forward_reference(x[b], L, filt, ndim=ndim, do_swt=swt)
            for num, (r, (tol, noise)) in enumerate(zip(refs[b], tols)):
                g = plan.coeff_at(num, b).reshape(r.shape)
                err = float(np.abs(g.astype(np.float64) - r).max())
                _note(family, "fwd", err, noise)
                print("taps %-10s n=%2d %s L%d B%d fwd image %d band %d: err/noise = %.2f" % (family, n, shape, L, batch, b, num, _ratio(err, noise)))
                assert err <= tol, (tag, "forward", b, num, err, tol, noise)
        # the inverse on its own: the oracle's coefficients (image 0's for the images in between)
        for num in range(plan.nbands):
            band = np.stack([refs.get(b, refs[0])[num] for b in range(batch)]).astype(np.float32)
            assert plan._lib.pdwt_set_coeff(plan._h, band.ctypes.data_as(C.c_void_p), num, 0) == 0
        plan.reset_kernel_times()
        plan.inverse()
        inv = _launches(plan)
        print("taps %-10s n=%2d %s L%d B%d inv launches %s" % (family, n, shape, L, batch, inv))
        assert _served(inv, want_inv), (tag, "inverse ran", inv, "wanted", want_inv)
        for b in checked:
            want, (tol, noise) = tap_banks.inverse_reference(refs[b], shape, L, filt, ndim=ndim, do_swt=swt)
            g = plan.image_at(b).reshape(want.shape)
            err = float(np.abs(g.astype(np.float64) - want).max())
            _note(family, "inv", err, noise)
            print("taps %-10s n=%2d %s L%d B%d inv image %d: err/noise = %.2f" % (family, n, shape, L, batch, b, _ratio(err, noise)))
            assert err <= tol, (tag, "inverse", b, err, tol, noise)
        return L
    finally:
        plan.cleanup()


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    """Prints the largest err / noise per family and direction when the module is done (the table of profiles/taps_parity.txt)."""
    yield
    lines = ["taps-parity  K = %g (at most %g)" % (tap_banks.K, tap_banks.K_MAX)]
    lines += ["taps-parity  %-12s %s  max err/noise = %.2f" % (family, direction, ratio) for (family, direction), ratio in sorted(RATIOS.items())]
    print("\n" + "\n".join(lines))
    if os.environ.get("PDWT_TAPS_PARITY_OUT"):  # how profiles/taps_parity.txt is made
        with open(os.environ["PDWT_TAPS_PARITY_OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")


EVEN_LONG = list(range(22, 41, 2))
NO_PYR = ("PDWT_NO_PYRAMID", "PDWT_NO_TAIL")
SWT_STREAMS_OFF = (("swt_fwdstream", 0), ("swt_invstream", 0))


def swt_shapes(n, quad):
    """Two small images on which n taps get three levels (sides of 8 n >= 8 (n - 1)): 8 n + 5 rows, which no dilation divides (one
    chain of all rows), and 8 n rows (dilations 2 and 4 split them into 2 and 4 phases of their own); a width that is not whole
    quads (and wider than the 64 + 4 (n - 1) + 4 columns a staged window of level 3 needs) unless `quad`."""
    side = 8 * n
    return [(side + 5, side if quad else side + 2), (side, side if quad else side + 2)]


def three_levels(family, n, quad, want_fwd, want_inv):
    for i, shape in enumerate(swt_shapes(n, quad)):
        assert run_case(family, "swt2", n, shape, 3, 1, want_fwd, want_inv, seed=10 + i) == 3


# ---- 2D DWT -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EVEN_LONG)
def test_dwt2_long_strips(n):
    """dwt2_long_kernels.hpp, every even length: ragged strips and steps, fewer columns than a strip, rows the periodization wraps inside
    one warm-up, two levels; 16 columns x 32 rows under n taps (both axes wrap); a batch (the kernels take even sides only)."""
    with forced((("long_fwd", 110), ("long_inv", 110)), NO_PYR):
        for i, (shape, levels, batch) in enumerate([((136, 264), 2, 1), ((64, 72), 1, 1), ((96, 1032), 1, 1), ((256, 512), 2, 1), ((32, 16), 1, 1), ((64, 72), 1, 3)]):
            want_inv = ("dwt2_inv_level", "long")
            if shape == (136, 264) and n <= 34:  # two levels: the inverse of level 2 has 66 coefficient columns, not whole 16-B groups -- the tiles
                want_inv = [("dwt2_inv_level", "tile"), ("dwt2_inv_level", "long")]
            run_case("long", "dwt2", n, shape, levels, batch, ("dwt2_fwd_level", "long"), want_inv, seed=i)


@pytest.mark.parametrize("n", [22, 26, 32, 40])
def test_dwt2_tiles(n):
    """launch_dwt2_fast.hip without the strips: the small 32 x 16 / 32 x 8 shapes below 2^20 samples (odd sizes, axes shorter than the
    filter, a batch of odd images) and, 16 x 256^2 = 2^20 samples, the large 32 x 32 / 32 x 16 / 32 x 8 ones."""
    with forced((("long_fwd", 0), ("long_inv", 0)), NO_PYR):
        for i, (shape, levels, batch) in enumerate([((136, 264), 2, 1), ((61, 75), 1, 1), ((20, 36), 1, 1), ((75, 61), 1, 3), ((256, 256), 1, 16)]):
            run_case("tile", "dwt2", n, shape, levels, batch, ("dwt2_fwd_level", "tile"), ("dwt2_inv_level", "tile"), seed=i)


@pytest.mark.parametrize("n", [21, 39])
def test_dwt2_generic_odd_lengths(n):
    with forced((), NO_PYR):
        for i, (shape, levels, batch) in enumerate([((136, 264), 2, 1), ((61, 75), 1, 1), ((20, 36), 1, 1), ((75, 61), 1, 3)]):
            run_case("generic", "dwt2", n, shape, levels, batch, ("dwt2_fwd_level", "generic"), ("dwt2_inv_level", "generic"), seed=i)


@pytest.mark.parametrize("n", [22, 40])
def test_dwt2_tail_batch_mode(n):
    """dwt2_tail_kernels.hpp, one workgroup per image: a batch of 2^20 samples of images of at most 65536 / n samples (default dispatch);
    both axes shorter than 40 taps, an odd size, and 32 x 32 (the mask / shift kernels of power-of-two sizes)."""
    for i, (shape, batch) in enumerate([((32, 48), 700), ((31, 45), 760), ((32, 32), 1024)]):
        run_case("tail", "dwt2", n, shape, 1, batch, ("dwt2_fwd_tail", ""), ("dwt2_inv_tail", ""), seed=i)


# ---- 1D DWT -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [21, 22, 39, 40])
def test_dwt1_level_launches(n):
    """dwt1_kernels.hpp: one instantiation per even length, the any-length one (HLEN = 0) for 21 and 39 taps."""
    with forced((), ("PDWT_NO_FUSED_1D",)):
        for i, (shape, levels, batch) in enumerate([((3, 4128), 3, 1), ((2, 1001), 2, 1), ((3, 36), 1, 1), ((1, 1001), 2, 3)]):
            run_case("dwt1_level", "dwt1", n, shape, levels, batch, ("dwt1_fwd_level", ""), ("dwt1_inv_level", ""), seed=i)


@pytest.mark.parametrize("n", [22, 40])
def test_dwt1_fused_pyramids(n):
    """dwt1_fused_kernels.hpp (default dispatch): runs of levels out of LDS; a row shorter than the filter has one level and stays a
    level launch."""
    for i, (shape, levels, batch) in enumerate([((3, 4128), 3, 1), ((2, 4096), 3, 1), ((1, 2064), 2, 3)]):
        run_case("dwt1_fused", "dwt1", n, shape, levels, batch, ("dwt1_fwd_fused", ""), ("dwt1_inv_fused", ""), seed=i)
    run_case("dwt1_level", "dwt1", n, (3, 32), 1, 1, ("dwt1_fwd_level", ""), ("dwt1_inv_level", ""), seed=9)


# ---- 2D SWT -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EVEN_LONG)
def test_swt2_forward_stream(n):
    """swt_fwdstream_kernels.hpp, every even length, dilations 1, 2, 4: a width that is not whole quads, rows the dilation does not
    divide; 24 columns x 40 rows (both wrap); a batch of odd images.  A width that is not whole quads AND narrower than one staged
    window is declined: the any-length stream kernels serve it."""
    with forced((("swt_fwdstream", 106), ("swt_invstream", 0))):
        three_levels("fwdstream", n, False, ("swt2_fwd_stream", ""), ("swt2_inv_split", "stream"))
        run_case("fwdstream", "swt2", n, (135, 200), 1, 1, ("swt2_fwd_stream", ""), ("swt2_inv_split", "stream"), seed=1)
        run_case("fwdstream", "swt2", n, (40, 24), 1, 1, ("swt2_fwd_stream", ""), ("swt2_inv_split", "stream"), seed=2)
        run_case("fwdstream", "swt2", n, (67, 121), 1, 3, ("swt2_fwd_stream", ""), ("swt2_inv_split", "stream"), seed=3)
        run_case("split_stream", "swt2", n, (130, 70), 1, 1, ("swt2_fwd_split", "stream"), ("swt2_inv_split", "stream"), seed=4)


@pytest.mark.parametrize("n", [22, 24, 26, 28])
def test_swt2_inverse_stream(n):
    with forced((("swt_invstream", 106), ("swt_fwdstream", 0))):
        three_levels("invstream", n, False, ("swt2_fwd_split", "stream"), ("swt2_inv_stream", ""))
        run_case("invstream", "swt2", n, (135, 200), 1, 1, ("swt2_fwd_split", "stream"), ("swt2_inv_stream", ""), seed=1)
        run_case("invstream", "swt2", n, (40, 24), 1, 1, ("swt2_fwd_split", "stream"), ("swt2_inv_stream", ""), seed=2)
        run_case("invstream", "swt2", n, (67, 121), 1, 3, ("swt2_fwd_split", "stream"), ("swt2_inv_stream", ""), seed=3)
        run_case("split_stream", "swt2", n, (130, 70), 1, 1, ("swt2_fwd_split", "stream"), ("swt2_inv_split", "stream"), seed=4)


@pytest.mark.parametrize("n", EVEN_LONG)
def test_swt2_two_launch_stream(n):
    """swt_stream_kernels.hpp (the any-length kernels of the two-launch levels; the default for small images of 18 taps and more once
    the one-launch levels are off): any width."""
    with forced(SWT_STREAMS_OFF):
        three_levels("split_stream", n, False, ("swt2_fwd_split", "stream"), ("swt2_inv_split", "stream"))
        run_case("split_stream", "swt2", n, (40, 24), 1, 1, ("swt2_fwd_split", "stream"), ("swt2_inv_split", "stream"), seed=2)
        run_case("split_stream", "swt2", n, (67, 121), 1, 3, ("swt2_fwd_split", "stream"), ("swt2_inv_split", "stream"), seed=3)


@pytest.mark.parametrize("n", EVEN_LONG)
def test_swt2_two_launch_packed(n):
    """swt_split_kernels.hpp forced at every size (rows of whole quads), its column pass in registers."""
    with forced(SWT_STREAMS_OFF + (("swt_split_fwd", 110), ("swt_split_inv", 110), ("swt_colstream", 0))):
        three_levels("split_packed", n, True, ("swt2_fwd_split", "packed"), ("swt2_inv_split", "packed"))
        run_case("split_packed", "swt2", n, (40, 24), 1, 1, ("swt2_fwd_split", "packed"), ("swt2_inv_split", "packed"), seed=2)
        run_case("split_packed", "swt2", n, (67, 120), 1, 3, ("swt2_fwd_split", "packed"), ("swt2_inv_split", "packed"), seed=3)


@pytest.mark.parametrize("n", EVEN_LONG)
def test_swt2_two_launch_colstream(n):
    """... and its column pass streamed down strips (swt_colstream_kernels.hpp), a row count the dilation does not divide."""
    with forced(SWT_STREAMS_OFF + (("swt_split_fwd", 110), ("swt_split_inv", 110), ("swt_colstream", 110))):
        three_levels("colstream", n, True, ("swt2_fwd_split", "colstream"), ("swt2_inv_split", "colstream"))
        run_case("colstream", "swt2", n, (40, 24), 1, 1, ("swt2_fwd_split", "colstream"), ("swt2_inv_split", "colstream"), seed=2)
        run_case("colstream", "swt2", n, (67, 120), 1, 3, ("swt2_fwd_split", "colstream"), ("swt2_inv_split", "colstream"), seed=3)


@pytest.mark.parametrize("n", [21, 22, 39, 40])
def test_swt2_level_tiles(n):
    """swt_kernels.hpp: one instantiation per even length, the any-length one (HLEN = 0) for 21 and 39 taps."""
    with forced(SWT_STREAMS_OFF + (("swt_split_fwd", 0), ("swt_split_inv", 0))):
        three_levels("swt2_level", n, False, ("swt2_fwd_level", ""), ("swt2_inv_level", ""))
        run_case("swt2_level", "swt2", n, (40, 24), 1, 1, ("swt2_fwd_level", ""), ("swt2_inv_level", ""), seed=2)
        run_case("swt2_level", "swt2", n, (67, 121), 1, 3, ("swt2_fwd_level", ""), ("swt2_inv_level", ""), seed=3)


@pytest.mark.parametrize("n", [22, 40])
def test_swt2_tail_batch_mode(n):
    """swt2_tail_kernels.hpp: the whole transform of a tiny image per workgroup, batches of 2^20 samples (default dispatch); general and
    power-of-two sizes."""
    for i, (shape, batch) in enumerate([((32, 48), 700), ((31, 45), 760), ((32, 32), 1024)]):
        run_case("swt2_tail", "swt2", n, shape, 1, batch, ("swt2_fwd_tail", ""), ("swt2_inv_tail", ""), seed=i)


# ---- 1D SWT -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [21, 22, 26, 39, 40])
def test_swt1_row_kernels(n):
    """The row kernels of swt_split_kernels.hpp on rows of whole quads, the any-length stream kernels on the others, the
    four-samples-per-work-item kernels on a row shorter than 128 samples (and than the filter): dilations 1, 2, 4.  21 and 39 taps: the
    one-sample-per-thread pass (swt_pass_*_kernel) on rows of whole quads."""
    for i, (shape, levels, batch) in enumerate([((3, 4100), 3, 1), ((2, 4101), 3, 1), ((3, 36), 1, 1), ((1, 1001), 2, 3)]):
        run_case("swt1", "swt1", n, shape, levels, batch, ("swt1_fwd_level", ""), ("swt1_inv_level", ""), seed=i)


# ---- the families of at most 20 taps: one length each ---------------------------------------------------------------------------------

SHORT = [
    ("wave", "dwt2", 8, (256, 512), 2, (("wave_min_log2", 0), ("lds_max_log2", 0)), ("PDWT_NO_PYRAMID",), ("dwt2_fwd_level", "wave"), ("dwt2_inv_level", "wave")),
    ("ring", "dwt2", 16, (130, 260), 1, (("ring_min_log2", 0),), ("PDWT_NO_PYRAMID",), ("dwt2_fwd_level", "ring"), ("dwt2_inv_level", "ring")),
    ("pyr3", "dwt2", 8, (256, 192), 3, (), (), ("dwt2_fwd_pyr3", ""), ("dwt2_inv_pyr3", "")),
    ("swt_fused4", "swt2", 4, (64, 512), 2, (), (), ("swt2_fwd_fused", ""), ("swt2_inv_fused", "")),
    ("reg1d", "dwt1", 16, (1, 8192), 3, (("reg1d", 15),), (), ("dwt1_fwd_reg", ""), ("dwt1_inv_reg", "")),
]


@pytest.mark.parametrize("family,kind,n,shape,levels,keys,env,want_fwd,want_inv", SHORT, ids=[c[0] for c in SHORT])
def test_short_families_one_length_each(family, kind, n, shape, levels, keys, env, want_fwd, want_inv):
    with forced(keys, env):
        run_case(family, kind, n, shape, levels, 1, want_fwd, want_inv)
