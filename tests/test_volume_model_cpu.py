"""tests/volume_model.py without a GPU: the model is pinned to the references, the committed sequences meet their coverage
conditions, the refusal rules agree with the recorded refusals and with the table of docs/KERNELS.md, and the comparator that
tests/test_gpu_volume_sequences.py runs against the library catches every planted ordering defect (in the spirit of
tests/test_tap_banks_cpu.py: a check that cannot fail proves nothing)."""
import os
import re

import numpy as np
import pytest

import ops_ref
import volume_model as vm
import volume_ops_ref
import volume_prox_ref
import volume_ref
import volume_spin_ref
import volume_swt_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a, b):
    return all(ops_ref.same_bits(np.ascontiguousarray(x), np.ascontiguousarray(y)) for x, y in zip(a, b)) and len(a) == len(b)


# ------------------------------------------------------------------------------------------------------------ the table
def test_the_table_of_volumes_is_what_the_issue_asks_for():
    names = [s.name for s in vm.VOLUMES]
    assert len(set(names)) == len(names) and 10 <= len(names) <= 14
    shapes = {(s.shape, s.wname, s.asked) for s in vm.VOLUMES}
    assert set(volume_spin_ref.SHAPES) <= shapes
    assert sum(1 for s in vm.VOLUMES if s.cycle and not s.swt) == 2
    assert {s.segments for s in vm.VOLUMES if s.segments} == {1, 3} and not any(s.swt for s in vm.VOLUMES if s.segments)
    swt2 = [s for s in vm.VOLUMES if s.swt and s.levels == 2 and s.prec == "f32"]
    assert len(swt2) == 2 and any(s.shape[0] % 2 for s in swt2)  # dilation 2 does not divide the depth of one of them
    assert any(s.shape[0] % 2 for s in vm.VOLUMES if not s.swt) and any(s.shape[0] < s.hlen for s in vm.VOLUMES)
    assert {(s.swt, s.prec) for s in vm.VOLUMES} == {(0, "f32"), (1, "f32"), (0, "f64"), (1, "f64")}
    for s in vm.VOLUMES:
        assert int(np.prod(s.shape)) <= 8192, s  # a few thousand samples
        if s.segments:  # the forced segments cut every walk they can into several (dwt3_axis_kernels.hpp: dwt3_fwd_steps = div2(Nz))
            assert volume_ref.div2(s.shape[0]) > s.segments


# ------------------------------------------------------------------------------------------------- pinned to the references
@pytest.mark.parametrize("spec", vm.VOLUMES, ids=lambda s: s.name)
def test_the_models_transforms_are_the_references(spec):
    x = spec.image(3)
    m = vm.VolumeModel(spec, x)
    if spec.cycle:
        m.apply(("spin_on", spec.cycle))
    assert m.apply(("forward",)) == (0, None) and m.state == vm.FORWARD
    double = "full" if spec.prec == "f64" else False
    shifted = volume_spin_ref.shift(x, m.shift)
    if spec.swt:
        want = volume_swt_ref.forward(shifted, spec.wname, spec.levels, double)
    else:
        want = volume_ref.forward(shifted, spec.wname, spec.levels, double)
    assert bits(m.bands, want) and [b.shape for b in m.bands] == list(spec.band_shapes())
    assert bool(any(m.shift)) == bool(spec.cycle)
    assert m.apply(("soft", 40.0, 1, 1))[0] == 0
    thr = (volume_swt_ref if spec.swt else volume_ref).threshold(want, spec.levels, "soft", 40.0, 1, 1)
    assert bits(m.bands, thr)
    assert m.apply(("inverse",)) == (0, None) and m.state == vm.INVERSE and m.shift == (0, 0, 0)
    if spec.swt:
        rec = volume_swt_ref.inverse(thr, spec.wname, spec.levels, double)
    else:
        rec = volume_ref.inverse(thr, spec.shape, spec.wname, spec.levels, double)
    drawn = vm.start_state(spec).shift  # rolled back by what the forward drew; zeros without cycle spinning
    assert ops_ref.same_bits(m.image, np.ascontiguousarray(volume_spin_ref.shift(rec, [-v for v in drawn])))
    assert bits(m.bands, thr)  # the inverse leaves the coefficients alone


def test_the_models_operators_are_the_references():
    spec = vm.spec_named("dwt-5x7x11-haar-L2")
    m, t = vm.VolumeModel(spec, spec.image(1)), vm.VolumeModel(spec, spec.image(2))
    m.apply(("forward",)), t.apply(("forward",))
    b0 = m.bands
    m.apply(("group", 30.0, 1, 1))
    assert bits(m.bands, volume_prox_ref.group_soft(b0, 2, 30.0, 1, 1))
    b1 = m.bands
    assert m.apply(("group_norm", 1), t)[1] == float(volume_prox_ref.group_norm(b1, 2, 1))
    m.apply(("add_dst", -1.25), t)
    assert bits(m.bands, volume_prox_ref.axpy(b1, t.bands, -1.25))
    b2 = m.bands
    m.apply(("add_src", 0.5), t)
    assert bits(m.bands, b2) and bits(t.bands, volume_prox_ref.axpy(volume_ref.forward(spec.image(2), "haar", 2, False), b2, 0.5))
    rc, (sigma, table) = m.apply(("denoise", "BayesShrink", "soft", None, 1))
    want = volume_ops_ref.denoise(b2, spec.shape, "BayesShrink", "soft", None, True)
    assert rc == 0 and np.array_equal(sigma, want[0]) and ops_ref.same_bits(table, want[1]) and bits(m.bands, want[2])
    assert np.array_equal(m.apply(("read_band_stats",))[1], volume_ops_ref.band_stats(b2))
    b3 = m.bands
    rc, (thr, kept) = m.apply(("keep", 100, 0))
    want = volume_ops_ref.keep_largest(b3, 100, 0)
    assert rc == 0 and thr == want[0] and kept == want[1] and bits(m.bands, want[2])
    assert m.apply(("last_sparsify",))[1][1] == want[1]
    x = m.image
    m.apply(("set_image", 7, 0))
    assert m.state == vm.INIT and ops_ref.same_bits(m.image, spec.image(7))
    rc, _ = m.apply(("cycle_spin", "global", "hard", 40.0, 1, 0, 3))
    want = volume_spin_ref.cycle_spin(spec.image(7), "haar", 2, volume_spin_ref.lattice(3), "hard", 40.0, do_app=1)
    assert rc == 0 and m.state == vm.INVERSE and ops_ref.same_bits(m.image, np.ascontiguousarray(want)) and x is not m.image


def test_the_draws_are_splitmix64():
    # the first outputs of splitmix64 seeded with 0 and with 1234567 (Vigna's reference implementation)
    s, z = vm.splitmix64(0)
    assert z == 0xE220A8397B1DCDAF
    s, z = vm.splitmix64(s)
    assert z == 0x6E789E6AA1B965F4
    assert vm.splitmix64(1234567)[1] == 6457827717110365317


# ------------------------------------------------------------------------------------------------------------ refusals
def golden_spec(key):
    shape, wname, kind = key.split("-")
    return vm.VolumeSpec(key, tuple(int(n) for n in shape.split("x")), wname, 2, swt=1 if kind == "swt" else 0)


def test_the_refusals_are_the_recorded_ones():
    entries = vm.recorded_refusals()
    assert len(entries) >= 4 * 30 and {e[2] for e in entries} == {vm.FORWARD, vm.INVERSE}
    specs = {}
    codes = set()
    for key, label, state, op, recorded in entries:
        spec = specs.setdefault(key, golden_spec(key))
        m = vm.VolumeModel(spec, spec.image(1))
        m.apply(("forward",))
        if state == vm.INVERSE:
            m.apply(("inverse",))
        rc, _ = m.apply(op)
        assert rc == recorded, (key, label, rc, recorded)
        codes.add(recorded)
    assert {vm.ERR_STATE, vm.ERR_UNSUPPORTED, 0} <= codes
    # ... and the states the recording reads
    for key in specs:
        m = vm.VolumeModel(specs[key], specs[key].image(1))
        m.apply(("forward",)), m.apply(("inverse",))
        m.apply(("set_coeff", 1, 1, 0))
        assert m.state == vm.INVERSE
        m.apply(("set_coeff", 0, 1, 0))
        assert m.state == vm.FORWARD
        m.apply(("set_image", 1, 0))
        assert m.state == vm.INIT


CODES = {"PDWT_ERR_STATE": vm.ERR_STATE, "PDWT_ERR_UNSUPPORTED": vm.ERR_UNSUPPORTED, "0 values": 0}
SAMPLE = {"soft": ("soft", 1.0, 0, 0), "hard": ("hard", 1.0, 0, 0), "group": ("group", 1.0, 0, 0), "linf": ("linf", 1.0, 0),
          "shrink": ("shrink", 1.0, 0), "group_norm": ("group_norm", 0), "add_dst": ("add_dst", 1.0), "add_src": ("add_src", 1.0),
          "get_coeff": ("get_coeff", 1), "set_image": ("set_image", 1, 0), "set_coeff": ("set_coeff", 0, 1, 0), "circshift": ("circshift", 1, 2, 3),
          "spin_on": ("spin_on", 9), "cycle_spin": ("cycle_spin", "global", "soft", 1.0, 0, 0, 1), "estimate_sigma": ("estimate_sigma", 1),
          "threshold_bands": ("threshold_bands", 1, "soft", 0), "denoise": ("denoise", "VisuShrink", "soft", None, 1), "select": ("select", 1, 0),
          "keep": ("keep", 1, 0)}


def kernels_table():
    """rows of the table "What every volume entry point owes the state" of docs/KERNELS.md: [kinds, read, written, refusal, shift]"""
    with open(os.path.join(os.path.dirname(HERE), "docs", "KERNELS.md")) as f:
        text = f.read()
    part = text.split("What every volume entry point owes the state", 1)[1]
    rows = []
    for line in part.splitlines():
        if line.startswith("#") and rows:
            break
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) == 5 and cells[0].startswith("`"):
            rows.append([re.findall(r"`([a-z_]+)`", cells[0])] + cells[1:])
    return rows


def test_the_refusal_rules_are_the_table_of_the_kernel_document():
    rows = kernels_table()
    kinds = [k for r in rows for k in r[0]]
    assert sorted(kinds) == sorted(vm.KINDS), set(vm.KINDS) ^ set(kinds)
    dwt, swt = vm.spec_named("dwt-5x7x11-haar-L2"), vm.spec_named("swt-5x7x11-haar-L2")
    checked = 0
    for row_kinds, read, written, refusal, shift in rows:
        conds = [] if refusal == "never" else [tuple(p.strip() for p in part.split(":")) for part in refusal.split(",")]
        assert all(len(c) == 2 and c[1] in CODES and c[0] in ("stationary", "INVERSE", "FORWARD", "spinning", "shifted", "twin INVERSE") for c in conds), refusal
        for kind in row_kinds:
            op = SAMPLE.get(kind, (kind,))
            for spec in (dwt, swt):
                for state in vm.STATES:
                    for spinning, shifted in ((0, 0), (1, 0), (1, 1)):
                        for twin_state in (vm.FORWARD, vm.INVERSE):
                            st = vm.VolumeState(spec)
                            st.state, st.spinning, st.shift = state, bool(spinning), (1, 0, 2) if shifted else (0, 0, 0)
                            holds = {"stationary": spec.swt, "INVERSE": state == vm.INVERSE, "FORWARD": state == vm.FORWARD, "spinning": spinning,
                                     "shifted": shifted, "twin INVERSE": twin_state == vm.INVERSE}
                            want = next((CODES[code] for cond, code in conds if holds[cond]), None)
                            assert st.refusal(op, twin_state) == want, (kind, spec.name, state, spinning, shifted, twin_state)
                            checked += 1
                            if want is not None:
                                continue
                            st.advance(op)
                            after = {"-": state, "INIT": vm.INIT, "FORWARD": vm.FORWARD, "INVERSE": vm.INVERSE,
                                     "FORWARD (num 0 in INVERSE)": vm.FORWARD if state == vm.INVERSE else state}[written]
                            assert st.state == after, (kind, state, written)
                            if shift == "-":
                                assert st.shift == ((1, 0, 2) if shifted else (0, 0, 0)), (kind, shift)
                            elif shift == "zero" or (shift == "zero (spinning)" and spinning):
                                assert st.shift == (0, 0, 0), (kind, shift)
                            elif shift == "+ draw (spinning)" and spinning:
                                assert st.shift != ((1, 0, 2) if shifted else (0, 0, 0))
                            else:
                                assert shift in ("zero (spinning)", "+ draw (spinning)"), shift
    assert checked == len(vm.KINDS) * 2 * 3 * 3 * 2


# ------------------------------------------------------------------------------------------------------------ coverage
def of(spec, seeds=vm.SEEDS):
    return [vm.sequences()[(spec.name, seed)] for seed in seeds]


def walk(spec, ops):
    """[(tracker before the call as (state, spinning, shift, after_select), op, refusal code or None)]"""
    st = vm.start_state(spec)
    out = []
    for op in ops:
        rc = st.refusal(op)
        out.append(((st.state, st.spinning, st.shift, st.after_select), op, rc))
        if rc is None:
            st.advance(op)
    return out


def test_the_sequences_are_deterministic_and_of_full_length():
    seqs = dict(vm.sequences())
    assert len(seqs) == len(vm.VOLUMES) * (len(vm.SEEDS) + 1)
    for (name, seed), ops in seqs.items():
        spec = vm.spec_named(name)
        assert len(ops) == vm.LENGTH
        assert all(op[0] in (vm.CLASS_KINDS if seed == vm.CLASS_SEED else vm.KINDS) for op in ops)
    vm._SEQUENCES.clear()
    assert vm.sequences() == seqs
    text = vm.as_python(vm.VOLUMES[0], 1, seqs[(vm.VOLUMES[0].name, 1)], 3)
    assert text.count("\n    (") == 4 and "run_ops(spec, ops, seed=1)" in text
    compile(text, "<sequence>", "exec")


@pytest.mark.parametrize("spec", vm.VOLUMES, ids=lambda s: s.name)
def test_every_kind_is_called_in_every_state_and_every_refusal_is_reached(spec):
    seen = vm.covered_pairs(spec, of(spec))
    missing = [(vm.STATE_NAMES[s], k) for s in vm.STATES for k in vm.KINDS if (s, k) not in seen]
    assert not missing, missing
    steps = [w for ops in of(spec) for w in walk(spec, ops)]
    # every refusal the rules can produce for this kind of volume in a state is produced, and every kind that can run there runs
    for state in vm.STATES:
        for kind in vm.KINDS:
            mine = [w for w in steps if w[0][0] == state and w[1][0] == kind]
            st = vm.VolumeState(spec)
            st.state = state
            always = st.refusal(SAMPLE.get(kind, (kind,)))
            if always is not None:
                assert all(w[2] == always for w in mine), (state, kind)
            elif kind != "spin_off":  # (that one also depends on the shift: below)
                assert any(w[2] is None for w in mine), (state, kind)
    # spin_off runs, and is refused while the image is shifted wherever a spinning forward can be followed by it
    assert any(w[1][0] == "spin_off" and w[2] is None for w in steps)
    if not spec.swt:
        runs = [w for w in steps if w[1][0] == "cycle_spin" and w[2] is None]
        assert {w[1][1] for w in runs} == {"global", "visu"}  # the global beta and the adaptive method both ran
        assert {w[0][0] for w in runs} == {vm.INIT, vm.INVERSE}  # ... from a set image and from a reconstructed one
        assert any(w[1][0] == "cycle_spin" and w[2] == vm.ERR_STATE and w[0][0] != vm.FORWARD and w[0][1] for w in steps) or not spec.cycle
    # the class sequence: every method in at least one state, and a forward, an inverse and a threshold that ran
    mine = walk(spec, vm.sequences()[(spec.name, vm.CLASS_SEED)])
    assert {w[1][0] for w in mine} == set(vm.CLASS_KINDS)
    ran = {w[1][0] for w in mine if w[2] is None}
    assert {"forward", "inverse", "get_image"} <= ran and ran & {"soft", "hard"}
    if not spec.swt:
        assert "cycle_spin" in ran


@pytest.mark.parametrize("spec", vm.VOLUMES, ids=lambda s: s.name)
def test_the_shared_select_workspace_is_exercised_in_both_orders(spec):
    kinds = [[op[0] for op in ops] for ops in of(spec)]
    pairs = {(a, b) for ks in kinds for a, b in zip(ks, ks[1:])}
    assert any(("estimate_sigma", k) in pairs for k in vm.SELECTS)
    assert any((k, "estimate_sigma") in pairs for k in vm.SELECTS)
    triples = {(a, b, c) for ks in kinds for a, b, c in zip(ks, ks[1:], ks[2:])}
    assert any(("estimate_sigma", k, "estimate_sigma") in triples for k in vm.SELECTS)
    if not spec.swt:  # ... and they ran: none of the three was refused
        steps = [w for ops in of(spec) for w in walk(spec, ops)]
        assert any(a[2] is None and b[2] is None and c[2] is None and (a[1][0], b[1][0], c[1][0]) == ("estimate_sigma", "keep", "estimate_sigma")
                   for a, b, c in zip(steps, steps[1:], steps[2:]))
        # an estimate that finds the workspace as select / keep left it
        assert any(w[1][0] == "estimate_sigma" and w[2] is None and w[0][3] for w in steps)
    # two thresholds in a row with different betas (a stationary volume stages its table through one pinned buffer)
    assert any(a[0] in ("soft", "hard") and b[0] in ("soft", "hard") and a[1] != b[1] for ops in of(spec) for a, b in zip(ops, ops[1:]))
    # the group threshold with and without A_L
    assert {op[2] for ops in of(spec) for op in ops if op[0] == "group"} == {0, 1}


@pytest.mark.parametrize("spec", [s for s in vm.VOLUMES if s.cycle], ids=lambda s: s.name)
def test_the_orderings_of_a_cycle_spinning_volume_occur(spec):
    steps = [w for ops in of(spec) for w in walk(spec, ops)]
    pairs = list(zip(steps, steps[1:]))
    shifted = lambda w: w[0][1] and any(w[0][2])
    # two forwards in a row, both drawing
    assert any(a[1][0] == b[1][0] == "forward" and a[0][1] and b[0][1] and a[2] is None for a, b in pairs)
    assert any(w[1][0] == "set_image" and shifted(w) for w in steps)
    assert any(w[1][0] == "spin_off" and shifted(w) and w[2] == vm.ERR_STATE for w in steps)
    assert any(a[1][0] == "circshift" and a[0][0] == vm.INVERSE and a[2] is None and b[1][0] in ("get_coeff", "get_image", "raw_read") for a, b in pairs)
    assert any(w[1][0] == "cycle_spin" and w[0][1] and w[0][0] != vm.FORWARD and w[2] == vm.ERR_STATE for w in steps)
    assert any(w[1][0] == "inverse" and shifted(w) and w[2] is None for w in steps)


# ------------------------------------------------------------------------------------------------------------ sensitivity
class NoUnshift(vm.VolumeModel):
    """the inverse does not shift the result back"""
    def inverse(self):
        self.advance(("inverse",))
        self.image = self.reconstruct(self.bands)
        return vm.OK


class NoAccumulation(vm.VolumeModel):
    """the draws of forwards in a row do not add up: the shift is the last draw"""
    def accumulate(self, d):
        return tuple(d)


class SetImageKeepsTheShift(vm.VolumeModel):
    def shift_after_set_image(self):
        return self.shift


class NoRearm(vm.VolumeModel):
    """set_coeff(.., 0) after an inverse leaves the state INVERSE"""
    def state_after_rearm(self):
        return vm.INVERSE


class CircshiftKeepsInverse(vm.VolumeModel):
    def state_after_circshift(self):
        return self.state


class CycleSpinEndsForward(vm.VolumeModel):
    def state_after_cycle_spin(self):
        return vm.FORWARD


class AddChangesItsSource(vm.VolumeModel):
    """add_wavelet scales the source's approximation too"""
    def add_wavelet(self, src, alpha):
        rc = vm.VolumeModel.add_wavelet(self, src, alpha)
        src.bands = [src.bands[0] * src.spec.dt(alpha)] + list(src.bands[1:])
        return rc


class SigmaAfterKeepIsTheKth(vm.VolumeModel):
    """estimate_sigma after select / keep finds their key in the shared workspace and returns the K-th magnitude"""
    def estimate_sigma(self, skip):
        if self.after_select:
            self.sigma = np.array([float(self.sparsify[0][0])], dtype=np.float64)
            return vm.OK
        return vm.VolumeModel.estimate_sigma(self, skip)


class GroupIgnoresTheApproximation(vm.VolumeModel):
    def group(self, beta, do_app, normalize):
        return vm.VolumeModel.group(self, beta, 0, normalize)


class StaleBeta(vm.VolumeModel):
    """a second threshold in a row is applied with the first call's beta (the staged table had not left the pinned buffer)"""
    last = None

    def apply(self, op, twin=None):
        if op[0] in ("soft", "hard") and self.refusal(op) is None:
            beta = self.last if self.last is not None else op[1]
            self.last = op[1]
            return vm.VolumeModel.apply(self, (op[0], beta) + tuple(op[2:]), twin)
        if self.refusal(op, twin.state if twin is not None else vm.FORWARD) is None:
            self.last = None
        return vm.VolumeModel.apply(self, op, twin)


class InverseWritesTheApproximation(vm.VolumeModel):
    """the inverse leaves its level-L reconstruction in sub-band 0, as the reference's does (wt.cu:272-275)"""
    def inverse(self):
        rc = vm.VolumeModel.inverse(self)
        self.bands = [self.bands[0] * self.spec.dt(0.5)] + list(self.bands[1:])
        return rc


class AddShowsTheIntermediates(vm.VolumeModel):
    """the intermediates add_wavelet scaled show in the next forward: A_L comes out scaled"""
    touched = False

    def add_wavelet(self, src, alpha):
        self.touched = True
        return vm.VolumeModel.add_wavelet(self, src, alpha)

    def forward(self):
        rc = vm.VolumeModel.forward(self)
        if self.touched and self.spec.levels > 1:
            self.bands = [self.bands[0] * self.spec.dt(1.5)] + list(self.bands[1:])
        return rc


DEFECTS = [NoUnshift, NoAccumulation, SetImageKeepsTheShift, NoRearm, CircshiftKeepsInverse, CycleSpinEndsForward, AddChangesItsSource,
           SigmaAfterKeepIsTheKth, GroupIgnoresTheApproximation, StaleBeta, InverseWritesTheApproximation, AddShowsTheIntermediates]
# the volumes whose sequences are tried, the likeliest first (a defect of the spinning needs a spinning volume)
ORDER = ["dwt-5x7x11-haar-L2-cycle", "dwt-5x7x11-haar-L2", "swt-5x7x11-haar-L2", "dwt-9x10x12-db2-L1-cycle", "dwt-9x10x12-db2-L1"]


def first_catch(defect):
    for name in ORDER:
        spec = vm.spec_named(name)
        for seed in vm.SEEDS:
            try:
                vm.run_sequence(spec, vm.sequences()[(name, seed)], vm.model_subject(defect), seed)
            except vm.Mismatch as e:
                return name, seed, str(e)
    return None


@pytest.mark.parametrize("spec", [vm.spec_named(n) for n in ORDER], ids=lambda s: s.name)
def test_the_model_agrees_with_itself(spec):
    """the comparator with the model standing in for the library: every sequence passes, every seen / bound is 0"""
    for seed in vm.SEEDS:
        stats = vm.run_sequence(spec, vm.sequences()[(spec.name, seed)], vm.model_subject(vm.VolumeModel), seed)
        assert stats["calls"] == vm.LENGTH + 2 and stats["refused"] > 0
        assert all(stats[k] <= 0.5 for k in ("forward", "inverse")) and stats["cycle_spin"] <= 0.25  # the fp32 composition itself
        assert all(stats[k] == 0 for k in ("group","add", "norms", "group_norm", "band_stats", "table"))


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda d: d.__name__)
def test_every_planted_defect_is_caught_by_a_committed_sequence(defect):
    caught = first_catch(defect)
    assert caught is not None, "no committed sequence tells %s from the model: the generator needs another condition" % defect.__name__
    name, seed, message = caught
    assert "run_ops(spec, ops, seed=%d)" % seed in message  # ... and prints as a script
    print("%s: caught by %s seed %d: %s" % (defect.__name__, name, seed, message.splitlines()[0]))
