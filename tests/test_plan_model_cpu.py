"""The eager plan model (tests/plan_model.py) pinned to the CPU oracle, and the conditions on the call sequences that
tests/test_gpu_sequences.py runs on the GPU, checked by running generator + model here, without one.

The conditions are on the INPUTS of the GPU test: if a seed violates one, the generator changes, not the cap."""
import hashlib
from collections import Counter

import numpy as np
import pytest

import adaptive_ref
import ops_ref
import plan_model as pm
import plan_stand_in
import sparsify_ref
from adaptive_check import left_out_pairs
from oracle import oracle

ALL_SEEDS = pm.SEEDS + (pm.CLASS_SEED,) + pm.NEW_SEEDS + (pm.CLASS_SEED_2,)


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle.build()


def spec_of(name):
    return [p for p in pm.PLANS if p.name == name][0]


# ------------------------------------------------------------------------------------------- the model against the oracle alone
@pytest.mark.parametrize("name", ["swt2-haar-64x96-L3", "dwt2-db4-256x256-L4", "dwt1-sym8-3x4096-L5", "swt1-db2-1x100-L2"])
def test_model_agrees_with_the_oracle_on_a_fixed_sequence(name):
    s = spec_of(name)
    x = s.image(7)
    m = pm.PlanModel(s, x)
    kw = dict(ndim=s.ndim, do_swt=s.swt)
    assert m.forward() == 0 and m.state == pm.FORWARD
    ref = oracle.forward(x[0], s.wname, s.levels, **kw)
    for g, r in zip(m.bands, ref):
        assert np.array_equal(g[0], r)
    for op, beta, do_app, norm in (("soft", 12.0, 0, 1), ("hard", 5.0, 1, 0), ("soft", -1.5, 1, 1)):
        assert getattr(m, op + "_threshold")(beta, do_app, norm) == 0 and m.state == pm.FORWARD
        ref = oracle.threshold(ref, s.shape, s.levels, op, beta, do_app, norm, **kw)
        for k, (g, r) in enumerate(zip(m.bands, ref)):
            assert ops_ref.same_bits(g[0], r), (op, k)
    assert m.shrink(0.25, 1) == 0
    ref = oracle.shrink(ref, s.shape, s.levels, 0.25, 1, **kw)
    for g, r in zip(m.bands, ref):
        assert ops_ref.same_bits(g[0], r)
    n1, n2 = oracle.norms(ref, s.shape, s.levels, **kw)  # the oracle sums in float32
    assert abs(m.norm1()[1] - n1) <= 1e-4 * n1 and abs(m.norm2sq()[1] - n2) <= 1e-4 * n2
    assert m.norms_async() == 0 and m.norms_slot == m.norms()
    before = [b.copy() for b in m.bands]
    assert m.inverse() == 0 and m.state == pm.INVERSE
    assert np.array_equal(m.image[0], oracle.inverse(ref, s.shape, s.wname, s.levels, **kw))
    assert all(np.array_equal(a, b) for a, b in zip(before, m.bands)), "the inverse leaves the coefficients alone"


def test_model_state_machine_and_return_values():
    s = spec_of("swt2-db2-72x80-L3")
    m = pm.PlanModel(s, s.image(3))
    assert m.state == pm.INIT and m.get_coeff(1)[0] == 72 * 80  # legal before any forward: the zeroed arena
    m.forward()
    t = m.clone()
    assert t.state == pm.FORWARD and t.bands[0] is not m.bands[0]
    assert m.inverse() == 0 and m.inverse() == pm.ERR_STATE
    for rc in (m.soft_threshold(1.0), m.hard_threshold(1.0), m.group_soft_threshold(1.0), m.shrink(1.0), m.proj_linf(1.0),
               m.soft_threshold_norms(1.0)):
        assert rc == pm.ERR_STATE
    assert m.get_coeff(0)[0] == 0 and m.get_coeff_at(2, 0)[0] == 0 and m.get_coeff_region()[0] == 0
    assert m.get_image()[0] == 72 * 80 and m.norm1()[0] == 0
    assert m.add_wavelet(t, 1.0) == 1 and t.add_wavelet(m, 1.0) == 1
    assert m.set_coeff(m.bands[3], 3) == 0 and m.state == pm.INVERSE
    assert m.set_coeff(m.bands[0], 0) == 0 and m.state == pm.FORWARD  # re-armed
    assert m.inverse() == 0 and m.set_image(s.image(4)) == 0 and m.state == pm.INIT
    assert m.get_coeff_region()[0] == m.region()[1] == 10 * 72 * 80
    assert m.add_wavelet(t, 0.5) == 0
    m.set_filters_forward(s.banks()[1], "custom")
    assert m.add_wavelet(t, 0.5) == -1
    other = pm.PlanModel(spec_of("swt2-db2-64x64-L2-bound"), np.zeros((1, 64, 64)))
    assert other.add_wavelet(t, 1.0) == -1  # the level count is compared first
    # the region: bands back to back, each padded to 64 values
    s = spec_of("swt2-db3-30x44-L2")
    m = pm.PlanModel(s, s.image(1))
    offs, total = m.region()
    assert offs == [k * 1344 for k in range(7)] and total == 7 * 1344 and 30 * 44 == 1320
    m.forward()
    flat = m.flat_region()
    assert not flat[1320:1344].any() and np.array_equal(flat[1344:1344 + 1320], m.bands[1].ravel())


def test_model_circshift_and_cycle_spinning():
    s = spec_of("swt2-sym4-64x64-L2-cycle")
    x = s.image(9)
    m = pm.PlanModel(s, x)
    m.circshift(5, -7, 0)
    assert np.array_equal(m.image, x)
    m.circshift(5, -7, 1)
    assert np.array_equal(m.image[0], oracle.circshift(x[0], 5, -7))
    m.set_image(x)
    m.forward(shift=(11, 50))
    assert np.array_equal(m.image[0], oracle.circshift(x[0], 11, 50)) and m.shift == (11, 50)
    assert np.array_equal(m.bands[2][0], oracle.forward(oracle.circshift(x[0], 11, 50), "sym4", 2, do_swt=1)[2])
    m.inverse()
    assert np.abs(m.image - x).max() < 7e-4
    t = m.clone()
    t.shift = (1, 2)
    m.set_coeff(m.bands[0], 0)
    t.set_coeff(t.bands[0], 0)
    assert m.add_wavelet(t, 1.0) == -4


def test_model_nonseparable_and_custom_banks():
    s = spec_of("dwt2-nonsep-48x56-L2")
    m = pm.PlanModel(s, s.image(2))
    b = s.banks()[0]
    m.set_filters_forward(b, "custom")
    m.set_filters_inverse(b)
    m.forward()
    f = [t.ravel() for t in b[1]]
    l1 = oracle.nonsep_forward_level(m.image[0], *f, s.hlen)
    l2 = oracle.nonsep_forward_level(l1[0], *f, s.hlen)
    for g, r in zip(m.bands, [l2[0]] + l1[1:] + l2[1:]):
        assert np.array_equal(g[0], r)
    m.inverse()
    assert m.image.shape == (1, 48, 56) and np.isfinite(m.image).all()
    s = spec_of("dwt2-custom9-64x68-L1")
    m = pm.PlanModel(s, s.image(2))
    assert m.dec[0] == 9 and m.forward() == 0 and m.bands[0].shape == (1, 32, 34)


# ------------------------------------------------------------------------------------------- the generator's conditions
@pytest.fixture(scope="module")
def runs():
    """every sequence of the GPU test through the model: {(plan, seed): [(op, situation before it, refused)]}"""
    out = {}
    for table_spec in pm.PLANS:
        for seed in ALL_SEEDS:
            spec = table_spec.single() if seed == pm.CLASS_SEED_2 else table_spec  # (generated for one image: the class has no batch)
            ops = pm.sequences()[(spec.name, seed)]
            assert ops == pm.sequences()[(spec.name, seed)] and len(ops) == pm.LENGTH
            rng = np.random.default_rng(seed)
            m = pm.PlanModel(spec, spec.image(100 + seed))
            if spec.custom or not spec.separable:
                m.apply(("filt_fwd", 0))
                m.apply(("filt_inv", 0))
            m.forward(shift=(3, 5))
            twin = m.clone()
            sit, custom, rows = pm.Situation(), False, []
            for op in ops:
                before, bands_before = sit.name(), m.bands
                rc, _ = m.apply(op, twin=twin, shift=tuple(int(v) for v in rng.integers(0, 60, 2)))
                no = pm.refused(op, rc)
                if op[0] == "denoise" and not no:
                    # the table rule of tests/adaptive_check.py leaves out at most one (band, image) pair per table, and is not
                    # defined where a band AND the noise level are zero: no committed sequence may ask for more
                    stats = m.stats_slot if op[1] == "BayesShrink" else None  # (the model took the sums of `bands_before` for it)
                    assert left_out_pairs(spec.dt, bands_before, m.sigma_slot, op[1], stats) <= 1, (spec, seed, op)
                    if op[1] == "BayesShrink":
                        assert all(stats[b, i, 1] > 0 or m.sigma_slot[i] > 0 for b in range(1, spec.nbands) for i in range(spec.batch)), (spec, seed, op)
                if not spec.cycle:  # (a cycle-spinning plan's add_wavelet also depends on the shifts the library draws)
                    assert no == sit.would_refuse(op[0], custom), (spec, seed, op)
                sit.step(op, custom)
                if op[0] == "filt_fwd":
                    custom = pm.bank_name(spec, op[1]) != pm.bank_name(spec, 0)
                assert (sit.state == m.state) or no, (spec, seed, op)
                rows.append((op, before, no))
            out[(spec.name, seed)] = rows
    return out


def test_sequences_are_deterministic_and_complete():
    assert len(pm.sequences()) == len(pm.PLANS) * len(ALL_SEEDS)
    spec = pm.PLANS[0]
    assert pm.generate(spec, 1) == pm.generate(spec, 1) and pm.generate(spec, 1) != pm.generate(spec, 2)
    for (name, seed), ops in pm.sequences().items():
        kinds = {pm.CLASS_SEED: pm.REFERENCE_KINDS, pm.CLASS_SEED_2: pm.CLASS_KINDS}.get(seed, pm.KINDS if seed in pm.SEEDS else pm.ALL_KINDS)
        assert all(op[0] in kinds for op in ops)
    assert "run_ops(spec, ops)" in pm.as_python(spec, 1, pm.sequences()[(spec.name, 1)], 3)


def test_the_old_seeds_sequences_are_byte_for_byte_what_they_were():
    """seeds 1-4 and CLASS_SEED are drawn from the kinds they were always drawn from; the digest is of the generator's output before
    the adaptive kinds existed"""
    old = {key: ops for key, ops in pm.sequences().items() if key[1] in pm.SEEDS + (pm.CLASS_SEED,)}
    assert len(old) == 5 * len(pm.PLANS)
    assert hashlib.sha256(repr(sorted(old.items())).encode()).hexdigest() == "5451552a63852deb3cdc322a31de9345e64362f54629cef427b831f644392b08"


def test_every_operation_kind_occurs_at_least_ten_times(runs):
    n = Counter(op[0] for (name, seed), rows in runs.items() if seed in pm.SEEDS for op, _, _ in rows)
    assert all(n[k] >= 10 for k in pm.KINDS), sorted(n.items(), key=lambda t: t[1])[:5]
    n = Counter(op[0] for (name, seed), rows in runs.items() if seed == pm.CLASS_SEED for op, _, _ in rows)
    assert all(n[k] >= 10 for k in pm.REFERENCE_KINDS), sorted(n.items(), key=lambda t: t[1])[:5]
    n = Counter(op[0] for (name, seed), rows in runs.items() if seed in pm.NEW_SEEDS for op, _, _ in rows)
    assert all(n[k] >= 10 for k in pm.ALL_KINDS), sorted(n.items(), key=lambda t: t[1])[:5]
    n = Counter(op[0] for (name, seed), rows in runs.items() if seed == pm.CLASS_SEED_2 for op, _, _ in rows)
    assert all(n[k] >= 10 for k in pm.CLASS_KINDS), sorted(n.items(), key=lambda t: t[1])[:5]


def test_every_call_follows_every_lazy_situation_at_least_twice(runs):
    """on the plans that defer (plan.cpp: can_defer_soft), through the C ABI"""
    n = Counter()
    for (name, seed), rows in runs.items():
        if spec_of(name).defers and seed in pm.SEEDS:
            n.update((before, op[0]) for op, before, _ in rows)
    missing = [(s, k, n[(s, k)]) for s in pm.SITUATIONS for k in pm.KINDS if n[(s, k)] < 2]
    assert not missing, missing
    n = Counter()
    for (name, seed), rows in runs.items():
        if spec_of(name).defers and seed in pm.NEW_SEEDS:
            n.update((before, op[0]) for op, before, _ in rows)
    missing = [(s, k, n[(s, k)]) for s in pm.SITUATIONS for k in pm.NEW_KINDS if n[(s, k)] < 2]
    assert not missing, missing
    assert sum(1 for p in pm.PLANS if p.defers) >= 10


def test_refusals_are_capped_and_transforms_run(runs):
    for (name, seed), rows in runs.items():
        no = sum(1 for _, _, r in rows if r)
        if not spec_of(name).cycle:
            assert no <= 0.25 * len(rows), (name, seed, no)
        for kind in ("forward", "inverse"):
            assert sum(1 for op, _, r in rows if op[0] == kind and not r) >= 3, (name, seed, kind)


def test_betas_matter():
    """0, below, inside and above the details' magnitudes, a negative one; normalize and do_app both ways"""
    seen, flags = Counter(), Counter()
    for ops in pm.sequences().values():
        for op in ops:
            if op[0] in ("soft", "hard", "group", "soft_norms"):
                seen[[k for k, v in pm.BETAS.items() if v == op[1]][0]] += 1
                flags[("app", op[2])] += 1
                flags[("normalize", op[3])] += 1
    assert all(seen[k] >= 10 for k in pm.BETAS), seen
    assert all(flags[(f, v)] >= 10 for f in ("app", "normalize") for v in (0, 1)), flags
    for spec in pm.PLANS:
        if spec.batch > 3:
            continue
        m = pm.PlanModel(spec, spec.image(101))
        if spec.custom or not spec.separable:
            m.apply(("filt_fwd", 0))
        m.forward()
        d = np.abs(np.concatenate([b.ravel() for b in m.bands[1:]]))
        assert pm.BETAS["above"] > d.max() and pm.BETAS["negative"] < 0 == pm.BETAS["zero"], spec
        assert 0.02 <= float((d > pm.BETAS["inside"]).mean()) <= 0.98, (spec, float((d > pm.BETAS["inside"]).mean()))
        assert float((d > pm.BETAS["below"]).mean()) >= 0.99, spec


# ------------------------------------------------------------------------------------------- the library's table against the model
# pypwt_amd/csrc/lazy_state.hpp, in the order of `enum class Entry`, and of its `Pending` and `Consumed`
ENTRIES = ("forward", "inverse", "soft", "eager_threshold", "norms", "read_stats", "band_sweep", "add_wavelet", "get_coeff",
           "coeff_ptr", "set_coeff", "set_image", "clone", "untouched")
KEEP, APPLY, DROP, CONSUME = 0, 1, 2, 3
C_KEEP, WRITE_BACK, C_DROP = 0, 1, 2
ENTRY_OF_KIND = {
    "forward": "forward", "inverse": "inverse", "soft": "soft", "soft_norms": "soft",
    "hard": "eager_threshold", "group": "eager_threshold", "shrink": "eager_threshold", "linf": "eager_threshold",
    "norm1": "norms", "norm2sq": "norms", "norms_async": "norms", "add_dst": "add_wavelet", "add_src": "add_wavelet",
    "get_coeff": "get_coeff", "get_coeff_at": "get_coeff", "get_region": "get_coeff", "raw_read": "coeff_ptr",
    "set_coeff": "set_coeff", "set_image": "set_image", "clone": "clone",
    "get_image": "untouched", "get_image_at": "untouched", "circshift": "untouched", "filt_fwd": "untouched", "filt_inv": "untouched",
    "band_stats": "read_stats", "estimate_sigma": "read_stats", "select": "read_stats",
    "threshold_bands": "band_sweep", "denoise": "band_sweep", "keep": "band_sweep",
    "read_band_stats": "untouched", "read_sigma": "untouched", "last_thresholds": "untouched", "last_sparsify": "untouched",
    "take_band": "set_coeff",  # (of this plan; pdwt_coeff_ptr settles the producer, whose lazy state the sequences never touch)
}


def test_the_librarys_lazy_state_table_is_the_models_and_the_documents():
    """Every Entry of lazy_state.hpp (what plan.cpp's settle() performs) against plan_model.Situation, kind by kind and situation
    by situation, and against the rows of docs/KERNELS.md for the entries the model has no kind for."""
    import ctypes as C

    import emu_util
    lib = emu_util.lib()
    rows, out = {}, (C.c_int * 3)()
    for i, name in enumerate(ENTRIES):
        assert lib.emu_lazy_row(i, out) == 0, name
        rows[name] = tuple(out)
    assert lib.emu_lazy_row(len(ENTRIES), out) == -1, "an Entry this test does not know"
    assert not [k for k in pm.ALL_KINDS if k not in ENTRY_OF_KIND], "a kind of the model without an Entry"

    def library(row, state, pending, consumed):
        """(pending, consumed) after settle() and, for Pending::consume, the success branch of pdwt_inverse"""
        refuses, p, c = row
        if refuses and state == pm.INVERSE:
            return True, pending, consumed
        if p == CONSUME:
            pending, consumed = False, consumed or pending
        elif p in (APPLY, DROP):
            pending = False
        if c in (WRITE_BACK, C_DROP):
            consumed = False
        return False, pending, consumed

    for kind in pm.ALL_KINDS:
        row = rows[ENTRY_OF_KIND[kind]]
        # soft / soft_norms with do_app: what the call owes the EARLIER threshold (without it the new one becomes pending, below)
        op = {"soft": (kind, 12.0, 1, 0), "soft_norms": (kind, 12.0, 1, 0), "set_coeff": (kind, 1, 5), "take_band": (kind, 1)}.get(kind, (kind,))
        for state in (pm.FORWARD, pm.INVERSE):
            for pending, consumed in ((False, False), (True, False), (False, True)):
                sit = pm.Situation()
                sit.state, sit.pending, sit.consumed = state, pending, consumed
                no = sit.would_refuse(kind, False)
                sit.step(op, False)
                want = library(row, state, pending, consumed)
                if (kind, state, consumed) == ("inverse", pm.FORWARD, True):
                    # The library reaches "consumed outside INVERSE" only through a failed un-shift (PDWT_INVERSE_ERROR), a state the
                    # model does not have: there the stored details still owe the threshold and the row keeps it; the model's
                    # inverse() assigns `consumed = pending`
                    assert want == (False, False, True) and (no, sit.pending, sit.consumed) == (False, False, False)
                    continue
                assert (no, sit.pending, sit.consumed) == want, (kind, state, pending, consumed)
    for kind in ("soft", "soft_norms"):  # the one place that defers: after the earlier threshold has been applied
        for pending in (False, True):
            sit = pm.Situation()
            sit.pending = pending
            sit.step((kind, 12.0, 0, 0), False)
            assert sit.pending and not sit.consumed and rows["soft"][1] == APPLY

    assert {ENTRY_OF_KIND[k] for k in pm.READ_STATS} == {"read_stats"} and {ENTRY_OF_KIND[k] for k in pm.BAND_SWEEP} == {"band_sweep"}
    assert rows["untouched"] == (0, KEEP, C_KEEP)


# ------------------------------------------------------------------------------------------- the adaptive and K-term kinds
def test_new_kinds_are_their_references_on_a_fixed_sequence():
    """band_stats, estimate_sigma, select, keep, threshold_bands, denoise, the slot readers and take_band against
    tests/adaptive_ref.py and tests/sparsify_ref.py called directly, with the return values and refusals of the header."""
    s = spec_of("swt2-db4-128x136-L3-b3")
    m = pm.PlanModel(s, s.image(7))
    for kind in pm.SLOT_READERS:  # nothing has written them
        rc, got = m.apply((kind,))
        assert rc == 0 and all(not np.any(g) for g in (got if isinstance(got, tuple) else (got,))), kind
    m.forward()
    twin = m.clone()
    bands = [b.copy() for b in m.bands]
    rc, got = m.apply(("band_stats",))
    assert rc == 0 and np.array_equal(got, adaptive_ref.band_stats(bands)) and got.shape == (10, 3, 2)
    for skip in (1, 0):
        rc, got = m.apply(("estimate_sigma", skip))
        assert rc == 0 and np.array_equal(got, adaptive_ref.estimate_sigma(bands[3], bool(skip)))
    n = s.swept_count(0)
    assert n == 9 * 128 * 136 and s.swept_count(1) == 10 * 128 * 136
    rc, got = m.apply(("select", (0, n // 4, n + 5), 0))
    want = sparsify_ref.select_magnitude(bands, (0, n // 4, n + 5), 0)
    assert rc == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0][0] == np.inf and got[1][2] == n
    assert all(ops_ref.same_bits(a, b) for a, b in zip(m.bands, bands)), "the read-only calls leave the coefficients alone"
    rc, got = m.apply(("keep", n // 4, 1))
    thr, kept, bands = sparsify_ref.keep_largest(bands, n // 4, 1)
    assert rc == 0 and np.array_equal(got[0], thr) and np.array_equal(got[1], kept)
    assert all(ops_ref.same_bits(a, b) for a, b in zip(m.bands, bands)) and np.array_equal(m.apply(("last_sparsify",))[1][1], kept)
    T = s.table(908)
    assert T.shape == (10, 3) and np.isnan(T[0]).all() and np.isnan(T[1:]).sum() == 1 and T[1, 0] == 0 and (T[9, 2] < 0) == (908 % 4 == 0)
    assert m.apply(("threshold_bands", 908, "hard", 0))[0] == 0
    bands = adaptive_ref.threshold_bands(bands, T, "hard")
    assert all(ops_ref.same_bits(a, b) for a, b in zip(m.bands, bands))
    assert ops_ref.same_bits(m.apply(("last_thresholds",))[1][1], T), "a host table is staged in the plan's own slot"
    assert m.apply(("threshold_bands", 909, "soft", 1))[0] == 0 and ops_ref.same_bits(m.table_slot, T), "... a device table is not"
    bands = adaptive_ref.threshold_bands(bands, s.table(909), "soft")
    for method, mode, sigma, skip in (("BayesShrink", "soft", None, 1), ("VisuShrink", "hard", 7.25, 0), ("BayesShrink", "hard", (3.0, 4.0, 5.0), 1)):
        before_stats = m.stats_slot
        rc, got = m.apply(("denoise", method, mode, sigma, skip))
        sg, T, out = adaptive_ref.denoise(bands, 2, 128 * 136, method, mode, sigma, bool(skip))
        assert rc == 0 and np.array_equal(got[0], sg) and ops_ref.same_bits(got[1], T)
        assert all(ops_ref.same_bits(a, b) for a, b in zip(m.bands, out))
        if method == "BayesShrink":
            assert np.array_equal(m.stats_slot, adaptive_ref.band_stats(bands))
        else:
            assert m.stats_slot is before_stats, "VisuShrink takes no sums"
        if sigma is not None:
            assert np.array_equal(sg, np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)))
        bands = out
    # take_band: the twin's band, bit for bit; band 0 after inverse() re-arms it
    assert m.apply(("take_band", 4), twin=twin) == (0, None) and ops_ref.same_bits(m.bands[4], twin.bands[4])
    assert m.inverse() == 0
    for op in (("keep", 5, 0), ("threshold_bands", 910, "soft", 0), ("denoise", "VisuShrink", "soft", None, 1)):
        table = m.table_slot
        assert m.apply(op) == (pm.ERR_STATE, None) and m.table_slot is table and m.state == pm.INVERSE, op
    for op in (("band_stats",), ("estimate_sigma", 1), ("select", 3, 1)):
        assert m.apply(op)[0] == 0 and m.state == pm.INVERSE, op
    assert m.apply(("take_band", 2), twin=twin)[0] == 0 and m.state == pm.INVERSE
    assert m.apply(("take_band", 0), twin=twin)[0] == 0 and m.state == pm.FORWARD and ops_ref.same_bits(m.bands[0], twin.bands[0])
    assert not m.clone().stats_slot.any() and not m.clone().sparsify_slot[1].any(), "a clone's workspace is its own: zeros"
    # the rows of a 1D plan are pooled: one image
    s = spec_of("dwt1-sym8-3x4096-L5")
    m = pm.PlanModel(s, s.image(7))
    m.forward()
    assert m.apply(("estimate_sigma", 1))[1].shape == (1,) and m.apply(("band_stats",))[1].shape == (6, 1, 2)
    assert s.swept_count(0) == sum(b.size for b in m.bands[1:])


def test_conditions_on_the_adaptive_sequences(runs):
    new = {key: rows for key, rows in runs.items() if key[1] in pm.NEW_SEEDS}
    # every refusal of a new kind is reached (PDWT_ERR_STATE of the three sweeps; no plan of PLANS is refused as unsupported)
    for kind in pm.BAND_SWEEP:
        assert sum(1 for rows in new.values() for op, _, no in rows if op[0] == kind and no) >= 2, kind
        assert sum(1 for rows in new.values() for op, _, no in rows if op[0] == kind and not no) >= 10, kind
    assert not [op for rows in new.values() for op, _, no in rows if no and op[0] in pm.READ_STATS + pm.SLOT_READERS + ("take_band",)]
    # K over {0, 1, N/4, N-1, N, N+5}; one K per image on a batched plan
    seen, per_image = set(), 0
    for (name, seed), rows in new.items():
        s = spec_of(name)
        for op, _, _ in rows:
            if op[0] in ("select", "keep"):
                n = s.swept_count(op[2])
                ks = op[1] if isinstance(op[1], tuple) else (op[1],)
                per_image += isinstance(op[1], tuple) and len(set(op[1])) > 1
                seen |= {{0: "0", 1: "1", n // 4: "N/4", n - 1: "N-1", n: "N", n + 5: "N+5"}.get(k, "other") for k in ks}
    assert seen >= {"0", "1", "N/4", "N-1", "N", "N+5"} and per_image >= 3, (seen, per_image)
    # tables from host and device memory, a negative entry; sigma estimated, one value, one per image
    tables = [(spec_of(name), op) for (name, seed), rows in new.items() for op, _, no in rows if op[0] == "threshold_bands" and not no]
    assert {op[3] for _, op in tables} == {0, 1} and {op[2] for _, op in tables} == {"soft", "hard"}
    assert any((s.table(op[1])[1:] < 0).any() for s, op in tables), "no table with a negative entry"
    sigmas = [op[3] for rows in new.values() for op, _, no in rows if op[0] == "denoise" and not no]
    assert any(isinstance(s, float) for s in sigmas) and any(isinstance(s, tuple) and len(s) > 1 for s in sigmas)
    # the generator sets the noise band before a denoise that estimates its noise level on details that may be zero
    # (Situation.dead): the estimate must not thin out -- at least two of each of (BayesShrink, VisuShrink) x skip_zeros, and two
    # per combination and seed on average
    estimated = Counter((op[1], op[4]) for rows in new.values() for op, _, no in rows if op[0] == "denoise" and not no and op[3] is None)
    assert all(estimated[(m, skip)] >= 2 for m in ("BayesShrink", "VisuShrink") for skip in (0, 1)), estimated
    assert sum(estimated.values()) >= 16, estimated
    # the noise estimate and the K-term select share a workspace: both orders on one plan with no transform in between, and three
    # host uploads (a table, noise levels, K) through the one pinned buffer back to back
    both = uploads = 0
    for rows in new.values():
        kinds = [op[0] for op, _, no in rows if not no]
        pairs = set(zip(kinds, kinds[1:]))
        both += bool(pairs & {("estimate_sigma", "keep"), ("estimate_sigma", "select")}) and bool(pairs & {("keep", "estimate_sigma"), ("select", "estimate_sigma")})
        for (a, _, _), (b, _, _), (c, _, _) in zip(rows, rows[1:], rows[2:]):
            uploads += (a[0] == "threshold_bands" and a[3] == 0 and b[0] == "denoise" and b[3] is not None and c[0] in ("keep", "select"))
    assert both >= len(pm.PLANS) and uploads >= len(pm.PLANS), (both, uploads)


@pytest.fixture(scope="module")
def judge():
    """test_gpu_sequences.run_ops, the comparator of the GPU test, with the model behind AbiPlan's interface as its subject"""
    import test_gpu_sequences as tgs

    def run(spec, ops, seed, defect=None):
        return tgs.run_ops(spec, ops, seed, subject=lambda sp, image: plan_stand_in.ModelSubject(sp, image, defect=defect))
    run.canned = tgs.canned_adaptive
    return run


SMALL = ["swt2-haar-64x96-L3", "swt2-db3-30x44-L2", "swt2-sym4-64x64-L2-cycle", "dwt2-custom9-64x68-L1", "dwt2-nonsep-48x56-L2",
         "swt2-haar-64x96-L3-f64", "swt1-db2-1x100-L2", "dwt1-sym8-3x4096-L5", "swt2-db4-128x136-L3-b3"]


@pytest.mark.parametrize("name", SMALL)
def test_the_comparator_accepts_the_model_itself(judge, name):
    """... on the sequences with the new kinds and on the named adaptive orderings: every check of the GPU test can be met, the
    table rule included (no entry of a committed sequence is 0 / 0)"""
    spec = spec_of(name)
    for seed in pm.NEW_SEEDS:
        judge(spec, pm.sequences()[(name, seed)], seed)
    judge(spec, judge.canned(spec), 9)


@pytest.mark.parametrize("defect", plan_stand_in.DEFECTS)
def test_planted_defects_are_caught(judge, defect):
    """each stand-in library with one defect fails the GPU test's comparator on a generated sequence of a small plan that defers"""
    caught, tried = [], 0
    for spec in pm.PLANS:
        if spec.defers and spec.batch <= 3 and spec.shape[0] * spec.shape[1] <= 1 << 15 and len(caught) < 2:
            for seed in pm.NEW_SEEDS:
                tried += 1
                try:
                    judge(spec, pm.sequences()[(spec.name, seed)], seed, defect)
                except AssertionError as e:
                    caught.append((spec.name, seed, str(e).splitlines()[0]))
    assert caught, defect
    print("PLANTED %s: caught on %d of %d sequences, first: %s" % (defect, len(caught), tried, caught[0][2][:160]))
