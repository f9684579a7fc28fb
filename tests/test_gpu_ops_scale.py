"""The coefficient operators at the sizes, types and values where streaming kernels go wrong, and the invariant they all lean on
(`pytest -m gpu`).

soft / hard / group_soft threshold, shrink, proj_linf, norm1, norm2sq, add_wavelet, soft_threshold_norms and norms_device sweep the
plan's arena with 16-byte accesses over PADDED ranges: every band is padded to 64 values, the padding is zeroed when the plan is
created and nothing may ever store anything but zero there (pypwt_amd/csrc/ops_kernels.hpp; docs/KERNELS.md "The padding
invariant").  No getter returns padding, so a transform kernel whose last 16-byte store runs past the band end would leave every
band equal to the oracle's and every norm wrong.  tests/test_gpu_ops.py has the operators on six plans of at most 7 680 values.

A  the padding is zero after forward() and after inverse() on every plan of the dispatch-coverage table, on PADDED_CASES (a plan
   per reachable (launch, family) pair whose bands ARE padded) and after every operator call below;
B  the element-wise operators bit for bit against tests/ops_ref.py (numpy, pinned to the C oracle by test_ops_ref_cpu.py) applied to
   the very values the plan holds, on plans where the grid-stride loops loop (2^24 values), every band is odd, the batch is large,
   the range is smaller than a workgroup; fp32 and fp64; add_wavelet within 1 ulp, group_soft within the project's bound;
C  the norms and soft_threshold_norms against exact sums with the bound recursive summation guarantees, not 1e-5;
D  signed zeros, +-beta and its neighbours, denormals, max, infinities, NaN through every operator for beta in
   {7.5, 0, a denormal, -1.0, 1e30}.

Every figure the bounds are compared with is printed with the prefix "OPS-SCALE" (run with -s to see them).
"""
import ctypes as C

import numpy as np
import pytest

import ops_ref
from dispatch_cases import CASES as DISPATCH_CASES
from oracle import oracle
from test_gpu_dispatch import REACHABLE

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


# ----------------------------------------------------------------------------- a plan with its arena geometry
class Plan(object):
    """A BatchedWavelets(64) plan of a dispatch_cases-style case (kind, wavelet, shape, levels, batch, precision) and the layout of
    its coefficient region as pdwt_coeff_region reports it."""

    def __init__(self, case, seed=None):
        from pypwt_amd import BatchedWavelets, BatchedWavelets64
        kind, w, shape, L, B, prec = case
        self.case = case
        self.ndim = 2 if kind in ("dwt2", "swt2") else 1
        self.swt = 1 if kind.startswith("swt") else 0
        self.dt = np.float64 if prec == "f64" else np.float32
        cls = BatchedWavelets64 if prec == "f64" else BatchedWavelets
        wname = "db4" if isinstance(w, tuple) else w
        self.p = cls(B, shape[0], shape[1], wname, L, do_swt=self.swt, ndim=self.ndim)
        self.lib, self.h, self.B = self.p._lib, self.p._h, B
        if isinstance(w, tuple):  # a custom bank of odd length, as tests/dispatch_cases.run_case sets it
            rng = np.random.default_rng(w[1])
            taps = [rng.standard_normal(w[1]).astype(self.dt) * 0.3 for _ in range(4)]
            rp = C.POINTER(C.c_double if prec == "f64" else C.c_float)
            ptr = [C.cast(t.ctypes.data, rp) for t in taps]
            null = C.cast(None, rp)
            assert self.lib.pdwt_set_filters_forward(self.h, b"custom", w[1], ptr[0], ptr[1], null, null) == 0
            assert self.lib.pdwt_set_filters_inverse(self.h, ptr[2], ptr[3], null, null) == 0
        self.L = self.p.levels
        self.per = 3 if self.ndim == 2 else 1
        nb = self.p.nbands
        offs = (C.c_longlong * nb)()
        self.total = int(self.lib.pdwt_coeff_region(self.h, offs, nb))
        self.offs = [int(o) for o in offs]
        self.elems = [int(self.lib.pdwt_coeff_count(self.h, k, None, None)) for k in range(nb)]
        ends = self.offs[1:] + [self.total]
        self.pads = [e - o - n for o, n, e in zip(self.offs, self.elems, ends)]
        assert self.offs[0] == 0 and all(0 <= p < 64 for p in self.pads) and all(o % 64 == 0 for o in self.offs), "layout rule"
        self.image = None
        if seed is not None:
            self.image = (oracle.hash_input((B,) + tuple(shape), seed, 100.0) - 50.0).astype(self.dt)  # mixed signs
            self.p.set_image(self.image)

    def close(self):
        self.p.cleanup()

    # levels whose detail bands (and band 0 for the last level) all have padding behind them
    def level_is_padded(self, l):
        idx = [self.per * (l - 1) + 1 + k for k in range(self.per)] + ([0] if l == self.L else [])
        return all(self.pads[i] > 0 for i in idx)

    def download(self, after_inverse=False):
        """The whole coefficient region, padding included."""
        out = np.empty(self.total, dtype=self.dt)
        if not after_inverse:
            assert self.lib.pdwt_get_coeff_region(self.h, out.ctypes.data) == self.total
        else:  # the getters refuse after inverse(); the pointer and the plain copy do not
            ptr = self.lib.pdwt_coeff_ptr(self.h, 0)
            assert ptr != 0 and self.lib.pdwt_copy(self.h, out.ctypes.data, C.c_void_p(ptr), self.total, 2) == 0
        return out

    def upload(self, flat):
        """Put a region read with download() back (padding included: it was checked when it was read)."""
        assert flat.dtype == self.dt and flat.size == self.total
        ptr = self.lib.pdwt_coeff_ptr(self.h, 0)  # also applies a threshold that is still pending
        assert ptr != 0 and self.lib.pdwt_copy(self.h, C.c_void_p(ptr), flat.ctypes.data, self.total, 1) == 0

    def bands(self, flat):
        return [flat[o:o + n] for o, n in zip(self.offs, self.elems)]

    def set_bands(self, bands):
        for k, b in enumerate(bands):
            b = np.ascontiguousarray(b, dtype=self.dt)
            assert b.size == self.elems[k] and self.lib.pdwt_set_coeff(self.h, b.ctypes.data, k, 0) == 0

    def padding(self, flat):
        return [flat[o + n:o + n + p] for o, n, p in zip(self.offs, self.elems, self.pads)]

    def check_padding(self, flat, what):
        """Part A: every value between the end of a band and the next band's offset compares equal to 0 (-0.0 passes; NaN does not)."""
        for k, pad in enumerate(self.padding(flat)):
            bad = np.flatnonzero(~(pad == 0))
            assert bad.size == 0, "%s %s: padding of band %d is not zero: %d of %d values, first at +%d = %r" % (
                self.case, what, k, bad.size, pad.size, bad[0], pad[bad[0]])

    def norms(self):
        """(sum |c|, sum c^2) through the two-double device slot."""
        assert self.lib.pdwt_norms_async(self.h, None) == 0
        return self.p.read_norms()

    def getter_norms(self):
        a, b = self.lib.pdwt_real(), self.lib.pdwt_real()
        assert self.lib.pdwt_norm1(self.h, C.byref(a)) == 0 and self.lib.pdwt_norm2sq(self.h, C.byref(b)) == 0
        return a.value, b.value

    def call(self, op, beta, do_app=0, normalize=0):
        lib, h = self.lib, self.h
        rc = {"soft": lambda: lib.pdwt_soft_threshold(h, beta, do_app, normalize),
              "hard": lambda: lib.pdwt_hard_threshold(h, beta, do_app, normalize),
              "linf": lambda: lib.pdwt_proj_linf(h, beta, do_app),
              "shrink": lambda: lib.pdwt_shrink(h, beta, do_app),
              "group": lambda: lib.pdwt_group_soft_threshold(h, beta, do_app, normalize),
              "soft+norms": lambda: lib.pdwt_soft_threshold_norms_async(h, beta, do_app, normalize, None)}[op]()
        assert rc == 0, (op, lib.pdwt_last_error())

    def reference(self, bands, op, beta, do_app=0, normalize=0):
        if op in ("soft", "hard", "linf", "soft+norms"):
            return ops_ref.threshold(bands, self.L, self.ndim, op[:4], beta, do_app, normalize)
        if op == "shrink":
            return ops_ref.shrink(bands, beta, do_app)
        return ops_ref.group_soft(bands, self.L, self.ndim, beta, do_app, normalize)[0]


def norms_bound(plan, ref):
    """Recursive summation of n terms in any order is off by at most (n - 1) u sum|terms|, u = 2^-53; the terms |x| and, for fp32 data,
    (double)x * x are exact.  The factor 2 covers the rounded squares of the fp64 library and the cross-lane steps; n is the swept
    (padded) length."""
    return 2.0 * plan.total * U53 * ref


def assert_bands_equal(plan, flat, ref, what):
    for k, (g, r) in enumerate(zip(plan.bands(flat), ref)):
        if not np.array_equal(g, r):
            bad = np.flatnonzero(g != r)
            raise AssertionError("%s %s: band %d differs from the reference in %d of %d values, first at %d: %r != %r" % (
                plan.case, what, k, bad.size, g.size, bad[0], g[bad[0]], r[bad[0]]))


# ----------------------------------------------------------------------------- part A: the padding invariant
# the odd-size plans of part B (their operators are tested below; here: the transforms next to their padding)
SCALE_CASES = [
    ("dwt2", "db4", (4096, 4096), 4, 1, "f32"),      # 2^24 values: 8 trips of the element-wise loop, 16 of the norms loop
    ("dwt2", "db2", (1001, 773), 2, 3, "f32"),       # level 1 of odd length, padding behind every band, a batch
    ("swt2", "haar", (1001, 1002), 5, 1, "f32"),     # 16 bands of 1 003 002 values, padding, the deferred-threshold plan kind
    ("swt2", "db4", (600, 800), 3, 4, "f32"),        # batched SWT: group_soft with do_app = 1 is legal
    ("dwt1", "haar", (1, 1 << 22), 20, 1, "f32"),    # 21 launches share the 1024 partial-sum slots of soft_threshold_norms
    ("dwt1", "db2", (8192, 64), 3, 1, "f32"),        # batched rows
    ("dwt1", "db3", (3, 251), 2, 1, "f32"),          # every range smaller than one workgroup
    ("swt1", "db2", (1, 100), 2, 1, "f32"),          # tiny 1D SWT
    ("dwt2", "db4", (64, 64), 3, 300, "f32"),        # many small images in one band
    ("dwt2", "db4", (2049, 1025), 3, 2, "f64"),      # > 2^22 doubles, every level odd x odd (2^k + 1), padding of up to 504 bytes
    ("swt2", "haar", (301, 515), 3, 1, "f64"),       # fp64 SWT
    ("dwt1", "sym8", (1, (1 << 20) + 2), 5, 1, "f64"),  # fp64 1D
]
REDUCED_ABOVE = 5 << 20  # plans with more values run (do_app, normalize) = (1, 1) and (0, 0) only (the download is the cost)

# For every (launch name, family) pair of test_gpu_dispatch.REACHABLE a plan on which the pair runs AND whose bands touched by that
# launch have padding behind them: 2 x odd sizes per level for the decimated transforms (4094 -> 2047; 4095 -> 2048 would not do), an
# odd rows * cols for the SWT.  Found with the default dispatch on an MI355X; test_padding_next_to_every_reachable_pair asserts both
# properties for every plan and prints the table.
PADDED_CASES = [
    # ---- fp32
    ("dwt1", "db4", (1, (1 << 24) - 64), 6, 1, "f32"),   # dwt1 reg + fused + level, both directions
    ("dwt2", "haar", (1025, 1025), 10, 1, "f32"),        # level tile, tail: 2^k + 1 stays odd at every level
    ("dwt2", ("custom", 9), (254, 258), 1, 1, "f32"),    # generic
    ("dwt2", "db2", (504, 496), 3, 1, "f32"),            # pyr3
    ("dwt2", "db4", (1020, 1016), 2, 1, "f32"),          # pyr2
    ("dwt2", "db4", (4098, 4100), 1, 3, "f32"),          # wave, both directions (above 2^25 samples in images of 2^24)
    ("dwt2", "sym8", (2050, 4100), 1, 4, "f32"),         # register ring (from 2^25 samples)
    ("dwt2", "db20", (4100, 4104), 1, 1, "f32"),         # strip-streaming long-filter kernels (from 2^24 samples)
    ("dwt2", "haar", (4100, 4112), 2, 3, "f32"),         # two forward levels on streaming strips (2 taps: from 2^25 samples, columns in 16s)
    ("swt2", "db2", (1023, 1016), 4, 1, "f32"),          # fused pairs, also on any size
    ("swt2", "db7", (1023, 2040), 6, 1, "f32"),          # level, one-launch stream levels, inverse column stream
    ("swt2", "db7", (2047, 4088), 6, 1, "f32"),          # forward split, packed
    ("swt2", "db7", (2049, 4100), 6, 1, "f32"),          # forward split with the streamed column pass (from 2^23 samples)
    ("swt2", "db10", (249, 70), 1, 1, "f32"),            # split on the stream kernels
    ("swt2", "db3", (29, 36), 2, 1, "f32"),              # inverse level
    ("swt2", "haar", (31, 30), 3, 2000, "f32"),          # one workgroup per image
    ("swt1", "db2", (1, 99), 2, 1, "f32"),
    # ---- fp64
    ("dwt2", "db4", (1016, 1008), 3, 1, "f64"),          # level tile + wave
    ("dwt2", "db2", (248, 240), 3, 1, "f64"),            # pyr3
    ("dwt2", "db10", (2052, 2056), 1, 1, "f64"),         # strip-streaming long-filter kernels (from 2^22 samples)
    ("dwt2", "db20", (1026, 1026), 1, 1, "f64"),         # the inverse as row + column launches (36 taps and more from 2^20 samples)
    ("dwt1", "sym8", (1, (1 << 20) - 32), 5, 1, "f64"),  # reg
    ("swt2", "db2", (29, 36), 2, 1, "f64"),              # level
    ("swt2", "db4", (255, 248), 2, 1, "f64"),            # one-launch stream levels
    ("swt2", "haar", (300, 507), 3, 1, "f64"),           # fused, any size
    ("swt2", "haar", (302, 516), 3, 1, "f64"),           # fused
    ("swt2", "db13", (511, 504), 2, 1, "f64"),           # split on the stream kernels
]

# REACHABLE pairs that no padded plan can reach, each with the rule ("file:line: ...") that admits the pair only for level sizes
# that are whole multiples of 64 samples.  Empty: every size rule of the dispatch is a lower bound ("from 2^k samples") or a
# divisibility of rows or columns by at most 16, and 2 x odd rows (or a batch that is not a multiple of 4) keep the band length off
# the multiples of 64 under all of them.
ALIGNED_ONLY = {
    "f32": {},
    "f64": {},
}


def _fill(plan):
    if plan.dt is np.float32:
        plan.p.fill_hash(4242, 255.0)
    else:
        shape, B = plan.case[2], plan.B
        plan.p.set_image(np.stack([oracle.hash_input(shape, 4242, index_offset=b * shape[0] * shape[1]).astype(np.float64) for b in range(B)]))


def _steps(plan):
    """[(first level, last level)] of the forward and of the inverse launch list (pdwt_schedule_string: "KIND[a-b]" or "KIND[a]")."""
    import re
    out = []
    for line in plan.p.schedule().splitlines():
        out.append([(int(a), int(b or a)) for a, b in re.findall(r"\[(\d+)(?:-(\d+))?\]", line)])
    return out


def pairs_on_padded_bands(plan):
    """Runs forward() and inverse() with the launches recorded and the padding checked after each.  Returns (all pairs that ran, the
    pairs whose launch touched only levels with padding behind every band).  A launch is matched with its schedule step when the two
    lists have the same length (no step fell back to other launches); otherwise it counts only if EVERY level is padded."""
    steps = _steps(plan)
    every = all(plan.level_is_padded(l) for l in range(1, plan.L + 1))
    _fill(plan)
    plan.p.enable_kernel_timing(True)
    ran, padded = set(), set()
    for d, go in enumerate((plan.p.forward, plan.p.inverse)):
        plan.p.reset_kernel_times()
        go()
        names = [n for n, _ in plan.p.kernel_times()]
        fams = plan.p.kernel_families()
        launches = [(n, f) for n, f in zip(names, fams) if n.split("_")[0] in ("dwt1", "dwt2", "swt1", "swt2")]
        ran |= set(launches)
        if len(launches) == len(steps[d]):
            for pair, (a, b) in zip(launches, steps[d]):
                if all(plan.level_is_padded(l) for l in range(a, b + 1)):
                    padded.add(pair)
        elif every:
            padded |= set(launches)
        plan.check_padding(plan.download(after_inverse=bool(d)), "after %s()" % ("inverse" if d else "forward"))
    plan.p.enable_kernel_timing(False)
    return ran, padded


ALL_LAYOUT_CASES = list(DISPATCH_CASES) + [c for c in SCALE_CASES if c not in DISPATCH_CASES]


@pytest.mark.parametrize("case", ALL_LAYOUT_CASES, ids=lambda c: "%s-%s-%dx%d-L%d-b%d-%s" % (c[0], c[1] if isinstance(c[1], str) else "custom", c[2][0], c[2][1], c[3], c[4], c[5]))
def test_padding_is_zero_after_forward_and_after_inverse(case):
    """Every plan of the dispatch-coverage table (imported, not copied: "every kernel family the default dispatch can reach") and the
    plans of part B.  After inverse() too: set_coeff(.., 0) re-arms the plan and forward() rewrites bands, not padding."""
    plan = Plan(case)
    try:
        if not any(plan.pads):
            return  # the layout leaves no padding in this plan (test_the_padding_check_is_not_vacuous counts the others)
        _fill(plan)
        plan.p.forward()
        plan.check_padding(plan.download(), "after forward()")
        plan.p.inverse()
        plan.check_padding(plan.download(after_inverse=True), "after inverse()")
    finally:
        plan.close()


def test_the_padding_check_is_not_vacuous():
    """By the layout rule only 11 plans of the dispatch table have a padded band at all; PADDED_CASES and the plans of part B are
    there for the rest.  Counted from pdwt_coeff_region, and the check itself is shown to see a value planted in padding."""
    padded = 0
    for case in DISPATCH_CASES:
        plan = Plan(case)
        padded += 1 if any(plan.pads) else 0
        plan.close()
    assert padded == 11, padded
    plan = Plan(("dwt2", "db2", (61, 59), 2, 1, "f32"), seed=3)
    try:
        plan.p.forward()
        flat = plan.download()
        plan.check_padding(flat, "after forward()")
        assert all(p > 0 for p in plan.pads)
        for value in (1.0, np.nan, -1e-45):
            dirty = flat.copy()
            dirty[plan.offs[1] + plan.elems[1]] = value
            with pytest.raises(AssertionError):
                plan.check_padding(dirty, "planted")
        flat[plan.offs[1] + plan.elems[1]] = -0.0  # harmless in every sweep
        plan.check_padding(flat, "-0.0")
    finally:
        plan.close()


def test_padding_next_to_every_reachable_pair():
    """PADDED_CASES: every (launch, family) pair of the dispatch table on a plan whose bands touched by that launch are padded; what
    cannot be reached that way must be listed in ALIGNED_ONLY with the rule that says why, and nothing else may be listed."""
    reached = {"f32": set(), "f64": set()}
    for case in PADDED_CASES:
        plan = Plan(case)
        try:
            ran, padded = pairs_on_padded_bands(plan)
            assert padded, (case, "no launch of this plan touches padded bands only", sorted(ran), plan.pads)
            reached[case[5]] |= padded
            print("OPS-SCALE padded plan %s: %s" % (case, sorted(padded)))
        finally:
            plan.close()
    for prec in ("f32", "f64"):
        never = REACHABLE[prec] - reached[prec]
        print("OPS-SCALE %s: %d of %d reachable pairs ran next to padding; not: %s" % (prec, len(REACHABLE[prec] & reached[prec]), len(REACHABLE[prec]), sorted(never)))
        listed = set(ALIGNED_ONLY[prec])
        assert never - listed == set(), (prec, "never ran on a padded plan and has no rule in ALIGNED_ONLY", sorted(never - listed))
        assert listed - never == set(), (prec, "listed in ALIGNED_ONLY but runs on a padded plan", sorted(listed - never))
        assert all(isinstance(rule, str) and ":" in rule for rule in ALIGNED_ONLY[prec].values())


# ----------------------------------------------------------------------------- parts B and C: one plan at a time, many operators
class State(object):
    pass


@pytest.fixture(scope="module", params=SCALE_CASES, ids=lambda c: "%s-%s-%dx%d-L%d-b%d-%s" % (c[0], c[1], c[2][0], c[2][1], c[3], c[4], c[5]))
def st(request):
    s = State()
    s.plan = plan = Plan(request.param, seed=1)
    plan.p.forward()
    s.flat0 = plan.download()  # (its padding is checked by test_b0_plan_properties, and after every operator call)
    s.bands0 = plan.bands(s.flat0)
    details = np.concatenate([np.abs(b) for b in s.bands0[1:]])
    s.beta = float(np.float32(0.1 * details.max()))  # about a tenth of the largest detail magnitude
    s.zeroed = float(np.mean(details <= s.beta))
    s.reduced = plan.total > REDUCED_ABOVE
    s.combos = [(1, 1), (0, 0)] if s.reduced else [(0, 0), (1, 0), (0, 1), (1, 1)]
    yield s
    plan.close()


def test_b0_plan_properties(st):
    """What the table of SCALE_CASES claims, asserted from pdwt_coeff_region."""
    plan, case = st.plan, st.plan.case
    plan.check_padding(st.flat0, "after forward()")
    values = sum(plan.elems)
    if case[2] == (4096, 4096):
        assert values == 1 << 24 and plan.total // 4 >= 8 * 2048 * 256  # eight trips of the element-wise loop ...
        assert plan.total // 4 >= 16 * 1024 * 256                        # ... and sixteen of the norms loop
    if case[2] == (1001, 773):
        assert all(n % 2 == 1 for n in plan.elems[1:4]) and all(p > 0 for p in plan.pads) and plan.B == 3
    if case[2] == (1001, 1002):
        assert len(plan.elems) == 16 and set(plan.elems) == {1003002} and all(p > 0 for p in plan.pads)
    if case[2] == (600, 800):
        assert plan.B == 4 and plan.swt and plan.elems[0] == plan.elems[1]
    if case[3] == 20:
        assert plan.L == 20 and len(plan.elems) == 21
        share = 1024 // (plan.L + 1)
        assert share == 48
        groups = [-(-(e - o) // 1024) for o, e in zip(plan.offs, plan.offs[1:] + [plan.total])]  # workgroups of 256 lanes x 4 values
        assert [g > share for g in groups[1:]] == [True] * 6 + [False] * 14 and groups[-1] == 1
    if case[2] == (3, 251):
        assert max(plan.elems) < 1024
    if case[2] == (64, 64):
        assert plan.B == 300 and plan.elems[1] == 300 * 32 * 32
    if case[2] == (2049, 1025):
        assert plan.dt is np.float64 and values > 1 << 22 and all((n // 2) % 2 == 1 for n in plan.elems) and all(p > 0 for p in plan.pads)
    if case[5] == "f64" and case[0] != "dwt2":
        assert any(plan.pads)
    # a real share of the detail values lands on each side of beta
    assert 0.05 <= st.zeroed <= 0.95, st.zeroed
    hard = ops_ref.threshold(st.bands0, plan.L, plan.ndim, "hard", st.beta)
    z = sum(int((h == 0).sum()) for h in hard[1:]) / float(sum(plan.elems[1:]))
    assert 0.05 <= z <= 0.95, z


def _run(st, op, beta, do_app=0, normalize=0):
    plan = st.plan
    plan.upload(st.flat0)
    plan.call(op, beta, do_app, normalize)
    flat = plan.download()
    plan.check_padding(flat, "after %s(%r, %d, %d)" % (op, beta, do_app, normalize))
    return flat


def test_b1_elementwise_operators_bit_for_bit(st):
    """soft, hard, proj_linf, shrink: one IEEE subtraction, comparison, min / max or multiplication per value and no fast-math flag in
    the build: np.array_equal with the numpy reference on every band."""
    plan = st.plan
    for op in ("soft", "hard"):
        for do_app, normalize in st.combos:
            flat = _run(st, op, st.beta, do_app, normalize)
            assert_bands_equal(plan, flat, plan.reference(st.bands0, op, st.beta, do_app, normalize), "%s(%d, %d)" % (op, do_app, normalize))
    for op in ("linf", "shrink"):
        for do_app in (0, 1):
            beta = st.beta if op == "linf" else 0.25
            flat = _run(st, op, beta, do_app)
            assert_bands_equal(plan, flat, plan.reference(st.bands0, op, beta, do_app), "%s(%d)" % (op, do_app))


# fp64 group_soft against the np.longdouble reference: the largest error measured on the fp64 plans of SCALE_CASES, relative to
# max(|band|, 1) as the fp32 bound is; asserted at 8 x that (one power of two for each of the about three roundings of
# sqrt, division and the final product)
GROUP_SOFT_F64_MEASURED = 2.15e-16  # swt2 haar 301 x 515 L3; 1.4e-16 and 1.8e-16 on the other two plans


def test_b2_group_soft_threshold(st):
    plan = st.plan
    worst = 0.0
    for normalize in (0, 1):
        for do_app in ((0, 1) if plan.swt else (0,)):  # the approximation band has the detail shape only for the SWT
            if st.reduced and plan.swt and do_app != normalize:
                continue
            flat = _run(st, "group", st.beta, do_app, normalize)
            ref = plan.reference(st.bands0, "group", st.beta, do_app, normalize)
            for k, (g, r) in enumerate(zip(plan.bands(flat), ref)):
                scale = max(float(np.abs(r).max()), 1.0)
                err = float(np.abs(g.astype(np.longdouble) - r.astype(np.longdouble)).max()) / scale
                worst = max(worst, err)
                tol = 5e-6 if plan.dt is np.float32 else 8 * GROUP_SOFT_F64_MEASURED
                assert err <= tol, (plan.case, do_app, normalize, k, err)
    print("OPS-SCALE group_soft %s: largest error / max(|band|, 1) = %.3g" % (plan.case, worst))


def test_b3_add_wavelet_within_one_ulp(st):
    """dst += 0.5 * src: the kernel's fused multiply-add rounds once, the reference in the wider type twice: at most 1 ulp apart."""
    plan = st.plan
    other = Plan(plan.case, seed=2)
    try:
        other.p.forward()
        src = other.bands(other.download())
        plan.upload(st.flat0)
        assert plan.lib.pdwt_add_wavelet(plan.h, other.h, 0.5) == 0
        flat = plan.download()
        plan.check_padding(flat, "after add_wavelet")
        worst = 0.0
        for k, (g, r) in enumerate(zip(plan.bands(flat), ops_ref.axpy(st.bands0, src, 0.5))):
            ulps = np.abs(g - r) / np.spacing(np.abs(r))
            worst = max(worst, float(ulps.max()))
            assert worst <= 1.0, (plan.case, k, worst)
        assert any(not np.array_equal(a, b) for a, b in zip(plan.bands(flat), st.bands0))
        print("OPS-SCALE add_wavelet %s: largest error %.3g ulp" % (plan.case, worst))
    finally:
        other.close()


def test_b4_batched_plan_equals_single_image_plans(st):
    """Image b of the batched result == the same operator on a one-image plan holding image b's coefficients, first and last image."""
    plan = st.plan
    if plan.B == 1:
        return
    kind, w, shape, L, B, prec = plan.case
    single = Plan((kind, w, shape, L, 1, prec), seed=9)
    try:
        single.p.forward()
        ops = [("soft", st.beta, 1, 1), ("hard", st.beta, 0, 1), ("linf", st.beta, 1, 0), ("shrink", 0.25, 0, 0),
               ("group", st.beta, plan.swt, 1), ("soft+norms", st.beta, 0, 1)]
        for op, beta, do_app, normalize in ops:
            flat = _run(st, op, beta, do_app, normalize)
            for b in sorted({0, B - 1}):
                mine = [band[b * (n // B):(b + 1) * (n // B)] for band, n in zip(st.bands0, plan.elems)]
                single.set_bands(mine)
                single.call(op, beta, do_app, normalize)
                got = single.download()
                single.check_padding(got, "single-image plan after %s" % op)
                for k, (g, n) in enumerate(zip(single.bands(got), plan.elems)):
                    assert np.array_equal(g, plan.bands(flat)[k][b * (n // B):(b + 1) * (n // B)]), (plan.case, op, b, k)
    finally:
        single.close()


def _check_norms(plan, got, bands, what, record):
    ref = ops_ref.norms(bands)
    for name, g, r in zip(("norm1", "norm2sq"), got, ref):
        bound = norms_bound(plan, r)
        print("OPS-SCALE %s %s %s: got %.17g, exact %.17g, error = %.3g x bound" % (plan.case, what, name, g, r, abs(g - r) / bound if bound else 0.0))
        record.append(abs(g - r) / bound if bound else 0.0)
        assert abs(g - r) <= bound, (plan.case, what, name, g, r, bound)
    return ref


def test_c1_norms_with_the_bound_of_recursive_summation(st):
    """norms_device / pdwt_norms_async against exact sums, before and after a threshold; the blocking getters return real_t: one more
    rounding (2^-24 or 2^-53 relative)."""
    plan = st.plan
    rec = []
    plan.upload(st.flat0)
    ref = _check_norms(plan, plan.norms(), st.bands0, "after forward()", rec)
    u = 2.0 ** -24 if plan.dt is np.float32 else U53
    for g, r in zip(plan.getter_norms(), ref):
        assert abs(g - r) <= norms_bound(plan, r) + u * r, (plan.case, g, r)
    plan.check_padding(plan.download(), "after norms")
    flat = _run(st, "hard", st.beta, 1, 1)
    _check_norms(plan, plan.norms(), plan.bands(flat), "after hard_threshold", rec)
    print("OPS-SCALE norms %s: largest error = %.3g x the asserted bound" % (plan.case, max(rec)))


def test_c2_soft_threshold_norms(st):
    """One sweep: the sums are those of the thresholded values (same bound), the coefficients afterwards are bit for bit the numpy
    reference's and what soft_threshold alone leaves."""
    plan = st.plan
    rec = []
    for do_app, normalize in st.combos:
        plan.upload(st.flat0)
        if plan.case[3] == 20 and normalize:
            plan.p.enable_kernel_timing(True)
            plan.p.reset_kernel_times()
        plan.call("soft+norms", st.beta, do_app, normalize)
        got = plan.p.read_norms()
        if plan.case[3] == 20 and normalize:
            names = [n for n, _ in plan.p.kernel_times()]
            plan.p.enable_kernel_timing(False)
            # one stamp spans the L + 1 partial launches and the final sum; that the slots are really shared out on this plan is
            # asserted from the layout in test_b0_plan_properties (six ranges above the share of 48 workgroups, fourteen below)
            assert names == ["soft_threshold+norms"], names
        flat = plan.download()  # (applies the threshold a 2D SWT plan deferred)
        what = "soft_threshold_norms(%d, %d)" % (do_app, normalize)
        plan.check_padding(flat, "after " + what)
        ref = plan.reference(st.bands0, "soft", st.beta, do_app, normalize)
        assert_bands_equal(plan, flat, ref, what)
        _check_norms(plan, got, ref, what, rec)
        alone = _run(st, "soft", st.beta, do_app, normalize)
        assert np.array_equal(alone, flat), (plan.case, what, "differs from soft_threshold alone")
    print("OPS-SCALE soft_threshold_norms %s: largest error = %.3g x the asserted bound" % (plan.case, max(rec)))


def test_c3_deferred_soft_threshold_norms_compose(st):
    """2D SWT: the threshold stays deferred (the sweep only reads), the sums are the thresholded ones, and a second call composes with
    the first as two successive soft thresholds do: the coefficients read afterwards were thresholded exactly once by each."""
    plan = st.plan
    if not (plan.swt and plan.ndim == 2):
        return
    rec = []
    for normalize in ((1,) if st.reduced else (0, 1)):
        plan.upload(st.flat0)
        b1, b2 = st.beta, 0.37 * st.beta
        plan.call("soft+norms", b1, 0, normalize)
        got1 = plan.p.read_norms()
        plan.call("soft+norms", b2, 0, normalize)
        got2 = plan.p.read_norms()
        once = plan.reference(st.bands0, "soft", b1, 0, normalize)
        twice = plan.reference(once, "soft", b2, 0, normalize)
        _check_norms(plan, got1, once, "deferred soft_threshold_norms", rec)
        _check_norms(plan, got2, twice, "second deferred soft_threshold_norms", rec)
        flat = plan.download()
        plan.check_padding(flat, "after two deferred thresholds")
        assert_bands_equal(plan, flat, twice, "two deferred thresholds")


# ----------------------------------------------------------------------------- part D: edge values and unusual betas
EDGE_CASES = [(kind, w, shape, L, 1, prec) for prec in ("f32", "f64")
              for kind, w, shape, L in (("dwt2", "db2", (61, 59), 2), ("swt2", "haar", (40, 52), 2), ("dwt1", "sym4", (1, 301), 3))]
EDGE_BETA = 7.5


def _edge_betas(dt):
    return [EDGE_BETA, 0.0, float(np.finfo(dt).smallest_subnormal * dt(1000)), -1.0, 1e30]


@pytest.fixture(scope="module", params=EDGE_CASES, ids=lambda c: "%s-%s" % (c[0], c[5]))
def edge(request):
    plan = Plan(request.param, seed=4)
    plan.p.forward()
    plan.check_padding(plan.download(), "after forward()")
    assert any(plan.pads)
    yield plan
    plan.close()


def _edge_bands(plan, finite_only=False, no_max=False):
    vec = ops_ref.edge_vector(EDGE_BETA, plan.dt, finite_only=finite_only)
    if no_max:
        vec = vec[np.abs(vec) < np.finfo(plan.dt).max]
    return [ops_ref.tile(np.roll(vec, k), n) for k, n in enumerate(plan.elems)]


def test_d1_edge_values_through_the_elementwise_operators(edge):
    """|x| == beta and its neighbours, signed zeros, denormals, max, infinities and NaN: np.array_equal(equal_nan=True) with the
    reference and the same sign on every zero.  shrink(-1.0) divides by zero and is left out."""
    plan = edge
    bands = _edge_bands(plan)
    for beta in _edge_betas(plan.dt):
        calls = [(op, a, n) for op in ("soft", "hard") for a in (0, 1) for n in (0, 1)] + [("linf", a, 0) for a in (0, 1)]
        if beta != -1.0:
            calls += [("shrink", a, 0) for a in (0, 1)]
        for op, do_app, normalize in calls:
            plan.set_bands(bands)
            plan.call(op, beta, do_app, normalize)
            flat = plan.download()
            what = "%s(%r, %d, %d)" % (op, beta, do_app, normalize)
            plan.check_padding(flat, "after " + what)
            ref = plan.reference(bands, op, beta, do_app, normalize)
            for k, (g, r) in enumerate(zip(plan.bands(flat), ref)):
                if not ops_ref.same_bits(g, r):
                    bad = np.flatnonzero(~((g == r) | (np.isnan(g) & np.isnan(r))) | (np.signbit(g) != np.signbit(r)) & (r == 0))
                    raise AssertionError("%s %s band %d: %r -> %r, expected %r" % (plan.case, what, k, bands[k][bad[:6]], g[bad[:6]], r[bad[:6]]))


def test_d2_edge_values_through_group_soft_and_the_norms(edge):
    """The finite part of the vector.  group_soft is compared where the sum of squares of the group is a normal number of the band's
    type with room for the square root's argument (the kernel squares in that type: below tiny / eps or above max the squares
    underflow to 0 or overflow to inf and the float64 / longdouble reference says nothing about them).  The norms vector of the fp64
    plans leaves +-max out: its square overflows the float64 sums on both sides."""
    plan = edge
    fi = np.finfo(plan.dt)
    bands = _edge_bands(plan, finite_only=True)
    for beta in _edge_betas(plan.dt):
        for normalize in (0, 1):
            for do_app in ((0, 1) if plan.swt else (0,)):
                plan.set_bands(bands)
                plan.call("group", beta, do_app, normalize)
                flat = plan.download()
                plan.check_padding(flat, "after group_soft(%r, %d, %d)" % (beta, do_app, normalize))
                ref, sumsq = ops_ref.group_soft(bands, plan.L, plan.ndim, beta, do_app, normalize)
                got = plan.bands(flat)
                for l in range(1, plan.L + 1):
                    ok = (sumsq[l - 1] > float(fi.tiny) / float(fi.eps)) & (sumsq[l - 1] < float(fi.max) / 4)
                    assert ok.sum() > ok.size // 2
                    for i in [plan.per * (l - 1) + 1 + k for k in range(plan.per)] + ([0] if do_app and l == plan.L else []):
                        g, r = got[i][ok].astype(np.longdouble), ref[i][ok].astype(np.longdouble)
                        tol = (5e-6 if plan.dt is np.float32 else 8 * GROUP_SOFT_F64_MEASURED) * np.maximum(np.abs(r), 1.0)
                        assert (np.abs(g - r) <= tol).all(), (plan.case, beta, do_app, normalize, i)
    bands = _edge_bands(plan, finite_only=True, no_max=plan.dt is np.float64)
    rec = []
    plan.set_bands(bands)
    _check_norms(plan, plan.norms(), bands, "edge vector", rec)
    for op, beta in (("soft", EDGE_BETA), ("hard", EDGE_BETA), ("soft", -1.0), ("linf", -1.0), ("soft+norms", -1.0)):
        # beta < 0: soft(0) = linf(0) = |beta|, the one case in which an operator does not map the padding onto itself
        plan.set_bands(bands)
        plan.call(op, beta, 1, 0)
        got = plan.p.read_norms() if op == "soft+norms" else None
        flat = plan.download()
        plan.check_padding(flat, "after %s(%r)" % (op, beta))
        assert_bands_equal(plan, flat, plan.reference(bands, op, beta, 1, 0), "%s(%r)" % (op, beta))
        _check_norms(plan, got or plan.norms(), plan.bands(flat), "edge vector after %s(%r)" % (op, beta), rec)


def test_d3_a_threshold_with_beta_not_negative_is_still_one_launch():
    """What keeps the padding clean after a negative beta must not cost the common case anything: soft_threshold(beta >= 0) without
    normalize on a decimated plan is ONE recorded launch, one per level with normalize, and no other launch is recorded."""
    plan = Plan(("dwt2", "db2", (61, 59), 2, 1, "f32"), seed=4)
    try:
        plan.p.forward()
        plan.p.enable_kernel_timing(True)
        for args, want in (((5.0, 0, 0), ["soft_threshold"]), ((5.0, 0, 1), ["soft_threshold"] * 2), ((5.0, 1, 0), ["soft_threshold"] * 2)):
            plan.p.reset_kernel_times()
            plan.call("soft", *args)
            assert [n for n, _ in plan.p.kernel_times()] == want, args
        plan.p.reset_kernel_times()
        plan.call("soft+norms", 5.0, 0, 0)
        assert [n for n, _ in plan.p.kernel_times()] == ["soft_threshold+norms"]
    finally:
        plan.close()


# ----------------------------------------------------------------------------- the compiled binding
def test_e1_operators_through_the_compiled_binding():
    """pycudwt.Wavelets when it is the Cython class: one plan of part B and the edge vector of part D, same expectations."""
    import pycudwt
    if pycudwt.binding != "cython":
        pytest.skip("pycudwt.binding is %r: the compiled (cython) binding pypwt_amd._cy has not been built" % pycudwt.binding)
    x = oracle.hash_input((1001, 773), 1, 100.0) - 50.0

    def flat_coeffs(w):
        c = w.coeffs
        return [c[0]] + [b for lvl in c[1:] for b in (lvl if isinstance(lvl, (list, tuple)) else [lvl])]

    def fresh():
        w = pycudwt.Wavelets(x, "db2", 2)
        w.forward()
        return w
    bands0 = [b.copy().ravel() for b in flat_coeffs(fresh())]
    beta = float(np.float32(0.1 * max(np.abs(b).max() for b in bands0[1:])))
    edge_bands = [ops_ref.tile(np.roll(ops_ref.edge_vector(EDGE_BETA, np.float32), k), b.size) for k, b in enumerate(bands0)]
    for bands, bt in ((bands0, beta), (edge_bands, EDGE_BETA), (edge_bands, -1.0)):
        for op, do_app, normalize in [("soft", 1, 1), ("soft", 0, 0), ("hard", 1, 1), ("hard", 0, 0), ("linf", 1, 0), ("shrink", 0, 0)]:
            if op == "shrink" and bt == -1.0:
                continue
            w = fresh()
            for k, b in enumerate(bands):
                w.set_coeff(b.reshape(flat_coeffs(w)[k].shape), k)
            if op in ("soft", "hard"):
                getattr(w, op + "_threshold")(bt, do_app, normalize)
                ref = ops_ref.threshold(bands, 2, 2, op, bt, do_app, normalize)
            elif op == "linf":
                w.proj_linf(bt, do_app)
                ref = ops_ref.threshold(bands, 2, 2, "linf", bt, do_app)
            else:
                w.shrink(bt, do_app)
                ref = ops_ref.shrink(bands, bt, do_app)
            got = [np.array(b).ravel() for b in flat_coeffs(w)]
            for k, (g, r) in enumerate(zip(got, ref)):
                assert ops_ref.same_bits(g, r), (op, bt, do_app, normalize, k)
            if bands is bands0:
                n1, n2 = ops_ref.norms(ref)
                total = sum(-(-b.size // 64) * 64 for b in ref)
                assert abs(w.norm1() - n1) <= (2 * total * U53 + 2.0 ** -24) * n1
                assert abs(w.norm2sq() - n2) <= (2 * total * U53 + 2.0 ** -24) * n2
