"""A stand-in for the library behind the interface of test_gpu_sequences.AbiPlan: the plan model itself, and variants of it with one
planted defect each, so that tests/test_plan_model_cpu.py can show without a GPU what the GPU test's comparator accepts and catches."""
import numpy as np

from plan_model import BAND_SWEEP, INVERSE, READ_STATS, PlanModel, Situation, bank_name

# --------------------------------------------------------------------------------------------------------------- a stand-in library
# Planted defects: what a library would answer that got one row of lazy_state.hpp or one argument wrong.  Each must make
# test_gpu_sequences.run_ops fail on a committed sequence (tests/test_plan_model_cpu.py), or the sequences could not see it.
DEFECTS = ("stats_skip_write_back",    # read_stats does not write a consumed threshold back
           "sweep_skips_pending",      # band_sweep does not apply a pending threshold first
           "keep_sweeps_band0",        # keep sweeps band 0 although do_app = 0
           "denoise_ignores_sigma",    # denoise with a given sigma uses the estimate
           "take_band_no_rearm")       # take_band of band 0 after inverse() leaves the state PDWT_INVERSE


class ModelSubject(object):
    """The model behind the interface of test_gpu_sequences.AbiPlan, so that run_ops can judge it as it judges the library.  It keeps
    what the eager model does not have -- the library's two lazy slots (a Situation) and `lag`, the details as the arena would
    hold them while a threshold is deferred or consumed -- only to act out a `defect`; without one it answers as the model."""
    lib = None

    def __init__(self, spec, image=None, defect=None, model=None):
        self.spec, self.defect = spec, defect
        self.m = model if model is not None else PlanModel(spec, image)
        self.sit = Situation()
        self.sit.state = self.m.state
        self.lag = None
        self.custom_name = False
        self.rng = np.random.default_rng(11)
        self.offs, self.total = self.m.region()
        self.elems = [self.m.elems(k) for k in range(spec.nbands)]
        self.parent = None
        self.quiet = False

    def close(self):
        pass

    def last_error(self):
        return "the stand-in library"

    def state(self):
        return self.m.state

    def shift(self):
        return self.m.shift

    def image(self):
        return self.m.image.copy()

    def region(self):
        n, flat = self.m.get_coeff_region()
        return n, (flat if flat is not None else np.zeros(self.total, dtype=self.spec.dt))

    def raw(self):
        return self.m.flat_region()

    def split(self, flat):
        return [flat[o:o + n] for o, n in zip(self.offs, self.elems)]

    def slots(self):
        m = self.m
        return {"band stats": m.stats_slot, "sigma": m.sigma_slot, "table": m.table_slot, "sparsify threshold": m.sparsify_slot[0],
                "kept": m.sparsify_slot[1]}

    def norms_slot(self):
        return np.array(self.m.norms_slot if self.m.norms_slot is not None else (0.0, 0.0))

    def call(self, op, twin):
        k, m, sit = op[0], self.m, self.sit
        lazy = self.spec.defers and not sit.would_refuse(k, self.custom_name)
        before = m.bands
        if self.defect == "keep_sweeps_band0" and k == "keep":
            op = (k, op[1], 1)
        if self.defect == "denoise_ignores_sigma" and k == "denoise":
            op = op[:3] + (None,) + op[4:]
        if lazy and self.defect == "sweep_skips_pending" and k in BAND_SWEEP and sit.pending:
            m.bands = self.lag                     # the threshold was dropped, not applied
        swapped = lazy and self.defect == "stats_skip_write_back" and k in READ_STATS and sit.consumed
        if swapped:
            m.bands = self.lag                     # the sums and the select see the stored details, which still lack it
        was = m.state
        rc, data = m.apply(op, twin=twin.m if twin is not None else None,
                           shift=tuple(int(v) for v in self.rng.integers(0, 60, 2)) if k == "forward" else (0, 0))
        if swapped:
            m.bands = before
        if self.defect == "take_band_no_rearm" and k == "take_band" and was == INVERSE:
            m.state = INVERSE
        if lazy and k in ("soft", "soft_norms") and not op[2] and op[1] >= 0:
            self.lag = before                      # (an earlier pending one has been applied: `before` holds it)
        sit.step(op, self.custom_name)
        if k == "filt_fwd":
            self.custom_name = bank_name(self.spec, op[1]) != bank_name(self.spec, 0)
        if k == "clone" and rc == 0:
            data = ModelSubject(self.spec, model=data)
        if k in ("get_coeff", "get_coeff_at") and data is None:
            data = np.full(1, 7.0, dtype=self.spec.dt)  # a refused getter leaves the caller's buffer alone
        return rc, data
