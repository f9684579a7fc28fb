"""An EAGER host model of one plan of include/pypwt_amd.h, and the generator of the call sequences it judges.

The library keeps two pieces of lazy state beside the reference's `state` enum (plan.hpp: `pending`, a soft threshold that the
fused 2D SWT inverse applies while it loads the details, and `consumed`, the write-back such an inverse still owes).  The
model has neither: every operator is applied to its bands at once, so whatever the library returns after ANY order of calls has
one right answer here.  tests/test_gpu_sequences.py drives both with the same calls; tests/test_plan_model_cpu.py pins the model
to the CPU oracle and checks the conditions on the generated sequences without a GPU.

What every method returns and the state it leaves are written down from the header and the reference lines it cites:

  forward             0, state FORWARD (wt.cu:236-269); with do_cycle_spinning the IMAGE is shifted in place first (wt.cu:242-246)
  inverse             PDWT_ERR_STATE and nothing done in state INVERSE (wt.cu:272-275), else 0, state INVERSE; the coefficients
                      are NOT modified (plan.hpp:13-16; the reference overwrites band 0); cycle spinning: un-shift (wt.cu:303)
  soft / hard / group_soft_threshold, shrink, proj_linf, soft_threshold_norms
                      PDWT_ERR_STATE in state INVERSE (wt.cu:309-312, 319-322, 330-333, 341-344, 350-353), else 0; the state
                      does not change (the reference never sets W_THRESHOLD either)
  norm1 / norm2sq / norms_async
                      0 in every state (wt.cu:368-416 have no state check): sums over the stored coefficients
  add_wavelet         -1 other wavelet name or level count, +1 either operand in state INVERSE, -2 other geometry, -3 SWT vs DWT,
                      -4 both cycle spinning with different shifts, in that order (wt.cu:622-655), else 0
  get_image(_at)      the element count, every state (wt.cu:419-422)
  get_coeff(_at), get_coeff_region
                      0 in state INVERSE (wt.cu:473-477), else the element count
  set_image           0, state INIT (wt.cu:425-431)
  set_coeff           0; band 0 in state INVERSE re-arms the inverse: state FORWARD (wt.cu:465 has it commented out)
  clone               a deep copy, state and shift included (wt.cu:191-222)
  circshift           0; the image is shifted when `inplace` (wt.cu:364-366), rows stay for 1D plans
  set_filters_*       0; forward also renames the wavelet (wt.cu:558-600)

and, without a reference counterpart, from the header alone (pypwt_amd.h:133-194) and lazy_state.hpp:

  band_stats, estimate_sigma, select
                      0 in every state (Entry::read_stats: a pending threshold is applied first, a consumed one written back
                      first -- the eager model has neither to do); the result goes to the plan's slot
  threshold_bands, denoise, keep
                      PDWT_ERR_STATE in state INVERSE with nothing done, slots included (Entry::band_sweep), else 0; the state does
                      not change.  denoise leaves sigma, (BayesShrink) the sums and the table in the slots, keep threshold and
                      kept; a HOST table of threshold_bands is staged in the table slot (plan.cpp: plan_sweep_bands), a device
                      table is read where it is
  read_band_stats, read_sigma, last_thresholds, last_sparsify
                      pdwt_adaptive_slots / pdwt_sparsify_slots + pdwt_copy: every state, zeros until a call has written them (a
                      clone's slots are its own: zeros)
  take_band(num)      pdwt_wait_for_stream(plan, pdwt_get_stream(twin)), then pdwt_set_coeff(plan, pdwt_coeff_ptr(twin, num), num,
                      1): set_coeff's row for the plan (band 0 re-arms the inverse), coeff_ptr's for the twin

PDWT_ERR_UNSUPPORTED: plan.cpp refuses the per-band operators for more than 96 bands, more than 65535 images, a band of 2^31 values
(ensure_adaptive) and the select for 2^32 swept values per image (select_magnitude_impl).  Non-separable, 1D and batched-1D plans
are served (the rows of a 1D plan are pooled into one image: its bands are (1, rows, cols) here too).  Plans of PLANS that are
refused: none -- the largest has 13 bands, 2000 images and 2^20 values per band.

Arithmetic: transforms through oracle.forward / oracle.inverse (fp64 plans: double="full"; the non-separable plan level by level
through oracle.nonsep_*_level), operators through tests/ops_ref.py, tests/adaptive_ref.py and tests/sparsify_ref.py.
"""
import numpy as np

import adaptive_ref
import ops_ref
import sparsify_ref
from oracle import oracle

INIT, FORWARD, INVERSE = 0, 1, 2
ERR_STATE = -4

# every operation kind the sequences draw from ("add_dst": the plan is the destination of add_wavelet, "add_src": its source)
KINDS = ("forward", "inverse", "soft", "hard", "group", "shrink", "linf", "norm1", "norm2sq", "norms_async", "soft_norms",
         "add_dst", "add_src", "get_image", "get_image_at", "get_coeff", "get_coeff_at", "get_region", "raw_read", "set_image",
         "set_coeff", "clone", "circshift", "filt_fwd", "filt_inv")
# ... and the ones the reference's Python class has a method for (src/pypwt.pyx:64-615)
REFERENCE_KINDS = ("forward", "inverse", "soft", "hard", "shrink", "norm1", "norm2sq", "add_dst", "add_src", "get_image",
                   "get_coeff", "get_region", "set_image", "set_coeff", "filt_fwd", "filt_inv")
# the adaptive and K-term calls (pypwt_amd.h:133-194), the readers of their result slots, and the documented hand-over of device
# data from one plan to another (take_band).  Seeds 1-5 are drawn from KINDS / REFERENCE_KINDS alone and stay what they were.
READ_STATS = ("band_stats", "estimate_sigma", "select")     # lazy_state.hpp: Entry::read_stats
BAND_SWEEP = ("threshold_bands", "denoise", "keep")         # ... Entry::band_sweep
SLOT_READERS = ("read_band_stats", "read_sigma", "last_thresholds", "last_sparsify")
NEW_KINDS = READ_STATS + BAND_SWEEP + SLOT_READERS + ("take_band",)
ALL_KINDS = KINDS + NEW_KINDS
# ... and the ones pypwt_amd.Wavelets has a method for (wavelets.py:158-295), beside the reference's
CLASS_KINDS = REFERENCE_KINDS + READ_STATS + BAND_SWEEP + SLOT_READERS
SITUATIONS = ("neither", "pending", "consumed")

# beta classes on images of 0..255 (checked against the first forward's details by test_plan_model_cpu.py):
# zero, below nearly every detail, inside their range, above all of them, negative (soft(0, b) = |b|: the padding is re-zeroed)
BETAS = {"zero": 0.0, "below": 1e-3, "inside": 12.0, "above": 1e6, "negative": -1.5}
SHRINK_BETAS = (0.25, 0.0, 3.0, -0.5)


class Spec(object):
    """One plan of the table of tests/test_gpu_sequences.py."""

    def __init__(self, name, kind, wname, shape, levels, batch=1, prec="f32", cycle=0, separable=1, custom=0, bound=False):
        self.name, self.kind, self.wname, self.shape, self.levels, self.batch = name, kind, wname, tuple(shape), levels, batch
        self.prec, self.cycle, self.separable, self.custom, self.bound = prec, cycle, separable, custom, bound
        self.ndim = 2 if kind.endswith("2") else 1
        self.swt = 1 if kind.startswith("swt") else 0
        self.dt = np.float64 if prec == "f64" else np.float32
        # plan.cpp: can_defer_soft
        self.defers = bool(self.swt and self.ndim == 2 and separable)
        self.hlen = custom if custom else oracle.filters(wname)[0]
        self.nbands = 1 + (3 if self.ndim == 2 else 1) * levels

    def __repr__(self):
        return self.name

    def banks(self):
        """Filter banks the sequences switch between; bank 0 is the plan's own (separable: (hlen, dec_lo, dec_hi, rec_lo,
        rec_hi); non-separable: (hlen, [LL, LH, HL, HH] forward, the same four for the inverse), hlen x hlen each)."""
        rng = np.random.default_rng(97 + self.hlen)
        if not self.separable:
            def four():
                return [(0.3 * rng.standard_normal((self.hlen, self.hlen))).astype(np.float32) for _ in range(4)]
            return [(self.hlen, four(), four()) for _ in range(3)]
        out = []
        if not self.custom:
            out.append(oracle.filters(self.wname, self.dt))
        for _ in range(3 - len(out)):
            out.append((self.hlen,) + tuple((0.3 * rng.standard_normal(self.hlen)).astype(self.dt) for _ in range(4)))
        return out

    def image(self, seed):
        """[batch][Nr][Nc] values of 0..255"""
        n = self.shape[0] * self.shape[1]
        return np.stack([oracle.hash_input(self.shape, seed, 255.0, index_offset=b * n) for b in range(self.batch)]).astype(self.dt)

    def band_shapes(self):
        nd = 1 if (self.ndim == 1 or self.shape[0] == 1) else 2
        return [(r, c) for (_, r, c) in oracle.Geometry(self.shape[0], self.shape[1], nd, self.swt, self.levels).bands]

    def level_of(self, num):
        return self.levels if num == 0 else ((num - 1) // 3 + 1 if self.ndim == 2 else num)

    def single(self):
        """the same plan for one image (the Python class has no batch)"""
        if self.batch == 1:
            return self
        return Spec(self.name, self.kind, self.wname, self.shape, self.levels, 1, self.prec, self.cycle, self.separable, self.custom, self.bound)

    def swept_count(self, do_app):
        """N of the K-term operators: the elements per image of the detail bands, and of band 0 with `do_app` (the rows of a 1D
        plan are pooled: they are one image)"""
        return sum(r * c for (r, c) in self.band_shapes()[0 if do_app else 1:])

    def table(self, seed):
        """[nbands][batch] thresholds of threshold_bands: 0.5 .. 30, NaN for the approximation and for one more (band, image), a
        zero, and for one seed in four a negative entry"""
        rng = np.random.default_rng([seed, 733])
        T = rng.uniform(0.5, 30.0, (self.nbands, self.batch)).astype(self.dt)
        T[0, :] = np.nan
        T[1 + int(rng.integers(0, self.nbands - 1)), int(rng.integers(0, self.batch))] = np.nan
        T[1, 0] = 0.0
        if seed % 4 == 0:
            T[self.nbands - 1, self.batch - 1] = -1.5
        return T


PLANS = [
    Spec("swt2-haar-64x96-L3", "swt2", "haar", (64, 96), 3),
    Spec("swt2-db2-72x80-L3", "swt2", "db2", (72, 80), 3),
    Spec("swt2-db4-128x136-L3-b3", "swt2", "db4", (128, 136), 3, batch=3),
    Spec("swt2-db10-250x78-L1", "swt2", "db10", (250, 78), 1),
    Spec("swt2-db10-250x1022-L2", "swt2", "db10", (250, 1022), 2),
    Spec("swt2-db3-30x44-L2", "swt2", "db3", (30, 44), 2),
    Spec("swt2-haar-32x32-L3-b2000", "swt2", "haar", (32, 32), 3, batch=2000),
    Spec("swt2-sym4-64x64-L2-cycle", "swt2", "sym4", (64, 64), 2, cycle=1),
    Spec("dwt2-db4-256x256-L4", "dwt2", "db4", (256, 256), 4),
    Spec("dwt2-db2-1001x773-L2", "dwt2", "db2", (1001, 773), 2),
    Spec("dwt2-db4-64x64-L3-b300", "dwt2", "db4", (64, 64), 3, batch=300),
    Spec("dwt1-sym8-3x4096-L5", "dwt1", "sym8", (3, 4096), 5),
    Spec("swt1-db2-1x100-L2", "swt1", "db2", (1, 100), 2),
    Spec("dwt2-custom9-64x68-L1", "dwt2", "db4", (64, 68), 1, custom=9),
    Spec("dwt2-nonsep-48x56-L2", "dwt2", "db2", (48, 56), 2, separable=0),
    Spec("swt2-haar-64x96-L3-f64", "swt2", "haar", (64, 96), 3, prec="f64"),
    Spec("dwt2-sym8-128x128-L2-f64", "dwt2", "sym8", (128, 128), 2, prec="f64"),
    Spec("swt2-db2-64x64-L2-bound", "swt2", "db2", (64, 64), 2, bound=True),
    # rows of 256 values and more: the fused groups (2 taps: levels 1-3, 4 taps: levels 1-2 in one launch; swt2_fused_supported)
    Spec("swt2-haar-64x256-L3", "swt2", "haar", (64, 256), 3),
    Spec("swt2-db2-40x264-L3", "swt2", "db2", (40, 264), 3),
]
SEEDS = (1, 2, 3, 4)   # the C-ABI sequences of every plan, drawn from KINDS
CLASS_SEED = 5         # the one through the Python class, drawn from REFERENCE_KINDS
NEW_SEEDS = (6, 7)     # C ABI, drawn from ALL_KINDS
CLASS_SEED_2 = 8       # the Python class, drawn from CLASS_KINDS
GIVEN_SIGMA = 7.25
LENGTH = 40


def pad64(n):
    return -(-n // 64) * 64


# --------------------------------------------------------------------------------------------------------------- the model
class PlanModel(object):
    def __init__(self, spec, image):
        self.spec = spec
        self.state = INIT
        self.image = np.array(image, dtype=spec.dt).reshape((spec.batch,) + spec.shape)
        self.shapes = spec.band_shapes()
        self.bands = [np.zeros((spec.batch,) + s, dtype=spec.dt) for s in self.shapes]  # the arena is zeroed at creation
        self.shift = (0, 0)
        self.wname = spec.wname
        banks = spec.banks()
        self.dec = self.rec = banks[0]
        self.norms_slot = None   # what norms_async / soft_threshold_norms left on the device: (sum |c|, sum c^2)
        self._clear_slots()
        self.input = None        # the image the last forward() was given (before the cycle-spinning shift)
        self.source = None       # ... while the bands are its untouched transform with the plan's own bank, else None

    def _clear_slots(self):
        """the plan's own result slots (pdwt_adaptive_slots, pdwt_sparsify_slots): the workspace is zeroed when it is allocated"""
        s = self.spec
        self.stats_slot = np.zeros((s.nbands, s.batch, 2), dtype=np.float64)
        self.sigma_slot = np.zeros(s.batch, dtype=np.float64)
        self.table_slot = np.zeros((s.nbands, s.batch), dtype=s.dt)
        self.sparsify_slot = (np.zeros(s.batch, dtype=s.dt), np.zeros(s.batch, dtype=np.uint64))

    # ---- layout
    def elems(self, num):
        return int(np.prod(self.bands[num].shape))

    def region(self):
        """(offset of every band, length): bands back to back in `num` order, each padded to 64 values (pypwt_amd.h)."""
        offs, at = [], 0
        for k in range(len(self.bands)):
            offs.append(at)
            at += pad64(self.elems(k))
        return offs, at

    def flat_region(self):
        offs, total = self.region()
        out = np.zeros(total, dtype=self.spec.dt)
        for o, b in zip(offs, self.bands):
            out[o:o + b.size] = b.ravel()
        return out

    # ---- arithmetic
    def _kw(self):
        s = self.spec
        return dict(ndim=s.ndim, do_swt=s.swt, double="full" if s.prec == "f64" else False)

    def transform(self, image):
        """oracle.forward of every image of the batch: bands as [batch][rows][cols]"""
        s = self.spec
        per_image = []
        for b in range(s.batch):
            x = image[b]
            if s.separable:
                per_image.append(oracle.forward(x, self.wname, s.levels, filt=(s.hlen, self.dec[1], self.dec[2], self.rec[3], self.rec[4]), **self._kw()))
            else:
                f = [t.ravel() for t in self.dec[1]]
                a, details = x, []
                for l in range(1, s.levels + 1):
                    a, h, v, d = oracle.nonsep_forward_level(a, f[0], f[1], f[2], f[3], s.hlen, do_swt=s.swt, level=l)
                    details += [h, v, d]
                per_image.append([a] + details)
        return [np.stack([pi[k] for pi in per_image]).reshape((s.batch,) + self.shapes[k]).astype(s.dt) for k in range(s.nbands)]

    def reconstruct(self, bands):
        s = self.spec
        out = []
        for b in range(s.batch):
            mine = [bd[b] for bd in bands]
            if s.separable:
                out.append(oracle.inverse(mine, s.shape, self.wname, s.levels, filt=(s.hlen, self.dec[1], self.dec[2], self.rec[3], self.rec[4]), **self._kw()))
            else:
                f = [t.ravel() for t in self.rec[2]]
                a = mine[0]
                for l in range(s.levels, 0, -1):
                    shape = s.shape if l == 1 else self.shapes[1 + 3 * (l - 2)]
                    a = oracle.nonsep_inverse_level([a] + mine[1 + 3 * (l - 1):4 + 3 * (l - 1)], shape, f[0], f[1], f[2], f[3], s.hlen,
                                                    do_swt=s.swt, level=l)
                out.append(a)
        return np.stack(out).reshape((s.batch,) + s.shape).astype(s.dt)

    def _shifted(self, image, sr, sc):
        if self.spec.ndim == 1:
            sr = 0
        return np.roll(image, (sr, sc), axis=(1, 2))  # common.cu:378-396: out[(r + sr) % Nr][(c + sc) % Nc] = in[r][c]

    # ---- transforms.  Both return what the oracle computes; the caller compares the library's result with it and hands the
    # library's in (`adopt_*`), so that everything between two transforms stays exact.
    def forward(self, shift=(0, 0)):
        self.input = self.image.copy()
        own = self.spec.banks()[0]
        same = self.spec.separable and all(np.array_equal(self.dec[i], own[i]) for i in (1, 2)) and \
            all(np.array_equal(self.rec[i], own[i]) for i in (3, 4))
        self.source = self.input if same else None
        if self.spec.cycle:
            self.shift = (int(shift[0]), int(shift[1]))
            self.image = self._shifted(self.image, *self.shift)
        self.bands = self.transform(self.image)
        self.state = FORWARD
        return 0

    def inverse(self):
        if self.state == INVERSE:
            return ERR_STATE
        self.image = self.reconstruct(self.bands)
        if self.spec.cycle:
            self.image = self._shifted(self.image, -self.shift[0], -self.shift[1])
        self.state = INVERSE
        return 0

    def adopt_bands(self, bands):
        self.bands = [np.array(b, dtype=self.spec.dt).reshape(m.shape) for b, m in zip(bands, self.bands)]

    def adopt_image(self, image):
        self.image = np.array(image, dtype=self.spec.dt).reshape(self.image.shape)

    # ---- operators
    def _flat(self):
        return [b.reshape(-1) for b in self.bands]

    def _store(self, flat):
        self.bands = [np.asarray(f, dtype=self.spec.dt).reshape(b.shape) for f, b in zip(flat, self.bands)]
        self.source = None

    def _threshold(self, op, beta, do_app, normalize):
        if self.state == INVERSE:
            return ERR_STATE
        self._store(ops_ref.threshold(self._flat(), self.spec.levels, self.spec.ndim, op, beta, do_app, normalize))
        return 0

    def soft_threshold(self, beta, do_app=0, normalize=0):
        return self._threshold("soft", beta, do_app, normalize)

    def hard_threshold(self, beta, do_app=0, normalize=0):
        return self._threshold("hard", beta, do_app, normalize)

    def proj_linf(self, beta, do_app=1):
        return self._threshold("linf", beta, do_app, 0)

    def group_soft_threshold(self, beta, do_app=0, normalize=0):
        if self.state == INVERSE:
            return ERR_STATE
        self._store(ops_ref.group_soft(self._flat(), self.spec.levels, self.spec.ndim, beta, do_app, normalize)[0])
        return 0

    def shrink(self, beta, do_app=1):
        if self.state == INVERSE:
            return ERR_STATE
        self._store(ops_ref.shrink(self._flat(), beta, do_app))
        return 0

    def norms(self):
        """(sum |c|, sum c^2): ops_ref.norms (exact sums) up to 2^20 values; above, numpy's pairwise sums in np.longdouble, whose
        own error (a few 2^-64 relative) is far inside the 2 n 2^-53 the library is held to"""
        flat = self._flat()
        if sum(b.size for b in flat) <= 1 << 20:
            return ops_ref.norms(flat)
        wide = [b.astype(np.longdouble) for b in flat]
        return float(sum(np.abs(w).sum() for w in wide)), float(sum((w * w).sum() for w in wide))

    def norm1(self):
        return 0, self.norms()[0]

    def norm2sq(self):
        return 0, self.norms()[1]

    def norms_async(self):
        self.norms_slot = self.norms()
        return 0

    def soft_threshold_norms(self, beta, do_app=0, normalize=0):
        rc = self.soft_threshold(beta, do_app, normalize)
        if rc == 0:
            self.norms_slot = self.norms()
        return rc

    def add_wavelet(self, src, alpha):
        """self += alpha * src"""
        a, b = self.spec, src.spec
        if a.levels != b.levels or self.wname.lower() != src.wname.lower():
            return -1
        if self.state == INVERSE or src.state == INVERSE:
            return 1
        if a.shape != b.shape or a.ndim != b.ndim or a.batch != b.batch:
            return -2
        if a.swt != b.swt:
            return -3
        if a.cycle and b.cycle and self.shift != src.shift:
            return -4
        self._store(ops_ref.axpy(self._flat(), src._flat(), alpha))
        return 0

    # ---- the adaptive and K-term calls: the arithmetic is tests/adaptive_ref.py's and tests/sparsify_ref.py's.  The read-only
    # ones are legal in every state; the sweeps return PDWT_ERR_STATE after inverse() with nothing done (pypwt_amd.h:162-165,
    # 183-185).  Each leaves its result in the plan's slot, where the readers find it.
    def band_stats(self):
        self.stats_slot = adaptive_ref.band_stats(self.bands)
        return 0

    def estimate_sigma(self, skip_zeros=1):
        self.sigma_slot = adaptive_ref.estimate_sigma(self.bands[adaptive_ref.noise_band(self.spec.ndim)], bool(skip_zeros))
        return 0

    def select(self, k, do_app=0):
        self.sparsify_slot = sparsify_ref.select_magnitude(self.bands, k, do_app)
        return 0

    def keep(self, k, do_app=0):
        if self.state == INVERSE:
            return ERR_STATE
        thr, kept, out = sparsify_ref.keep_largest(self.bands, k, do_app)
        self.sparsify_slot = (thr, kept)
        self._store(out)
        return 0

    def threshold_bands(self, table, op="soft", on_device=0):
        if self.state == INVERSE:
            return ERR_STATE
        if not on_device:  # plan.cpp, plan_sweep_bands: a host table is staged into the plan's own table slot
            self.table_slot = np.array(table, dtype=self.spec.dt)
        self._store(adaptive_ref.threshold_bands(self.bands, table, op))
        return 0

    def denoise(self, method="BayesShrink", op="soft", sigma=None, skip_zeros=1):
        if self.state == INVERSE:
            return ERR_STATE
        s = self.spec
        if method == "BayesShrink":  # plan.cpp, pdwt_denoise_async: the sums are taken for this recipe only
            self.stats_slot = adaptive_ref.band_stats(self.bands)
        sg, T, out = adaptive_ref.denoise(self.bands, s.ndim, s.shape[0] * s.shape[1], method, op, sigma, bool(skip_zeros))
        self.sigma_slot, self.table_slot = sg, T
        self._store(out)
        return 0

    def adopt_table(self, before, table, op):
        """denoise, second step: the sweep of `before` with the table the library made"""
        self.table_slot = np.array(table, dtype=self.spec.dt)
        self._store(adaptive_ref.threshold_bands(before, self.table_slot, op))

    def take_band(self, src, num):
        """pdwt_wait_for_stream(self, src's stream), then pdwt_set_coeff(self, pdwt_coeff_ptr(src, num), num, 1)"""
        return self.set_coeff(src.bands[num], num)

    # ---- data movement
    def get_image(self):
        return self.image.size, self.image

    def get_image_at(self, b):
        return self.image[b].size, self.image[b]

    def get_coeff(self, num):
        if self.state == INVERSE:
            return 0, None
        return self.bands[num].size, self.bands[num]

    def get_coeff_at(self, num, b):
        if self.state == INVERSE:
            return 0, None
        return self.bands[num][b].size, self.bands[num][b]

    def get_coeff_region(self):
        if self.state == INVERSE:
            return 0, None
        flat = self.flat_region()
        return flat.size, flat

    def set_image(self, image):
        self.adopt_image(image)
        self.state = INIT
        return 0

    def set_coeff(self, band, num):
        self.bands[num] = np.array(band, dtype=self.spec.dt).reshape(self.bands[num].shape)
        self.source = None
        if num == 0 and self.state == INVERSE:
            self.state = FORWARD
        return 0

    def clone(self):
        c = PlanModel.__new__(PlanModel)
        c.__dict__.update(self.__dict__)
        c.image = self.image.copy()
        c.bands = [b.copy() for b in self.bands]
        c.norms_slot = None
        c._clear_slots()
        return c

    def circshift(self, sr, sc, inplace):
        if inplace:
            self.image = self._shifted(self.image, sr, sc)
        return 0

    def set_filters_forward(self, bank, name):
        self.dec = bank
        self.wname = name
        self.source = None
        return 0

    def set_filters_inverse(self, bank):
        self.rec = bank
        self.source = None
        return 0

    # ---- one op of a generated sequence (tests/test_gpu_sequences.py applies the same op to the library)
    def apply(self, op, twin=None, shift=(0, 0)):
        """Returns (return value, data or None)."""
        k, a = op[0], op[1:]
        s = self.spec
        if k == "forward":
            return self.forward(shift), None
        if k == "inverse":
            return self.inverse(), None
        if k == "soft":
            return self.soft_threshold(*a), None
        if k == "hard":
            return self.hard_threshold(*a), None
        if k == "group":
            return self.group_soft_threshold(*a), None
        if k == "shrink":
            return self.shrink(*a), None
        if k == "linf":
            return self.proj_linf(*a), None
        if k == "norm1":
            return self.norm1()
        if k == "norm2sq":
            return self.norm2sq()
        if k == "norms_async":
            return self.norms_async(), self.norms_slot
        if k == "soft_norms":
            rc = self.soft_threshold_norms(*a)
            return rc, (self.norms_slot if rc == 0 else None)
        if k == "add_dst":
            return self.add_wavelet(twin, a[0]), None
        if k == "add_src":
            return twin.add_wavelet(self, a[0]), None
        if k == "get_image":
            return self.get_image()
        if k == "get_image_at":
            return self.get_image_at(a[0])
        if k == "get_coeff":
            return self.get_coeff(a[0])
        if k == "get_coeff_at":
            return self.get_coeff_at(a[0], a[1])
        if k == "get_region":
            return self.get_coeff_region()
        if k == "raw_read":
            return 0, self.flat_region()  # pdwt_coeff_ptr + pdwt_copy: legal in every state
        if k == "set_image":
            return self.set_image(new_image(s, a[0])), None
        if k == "set_coeff":
            return self.set_coeff(new_band(s, self.bands[a[0]].shape, a[1]), a[0]), None
        if k == "clone":
            return 0, self.clone()
        if k == "circshift":
            return self.circshift(*a), None
        if k == "filt_fwd":
            return self.set_filters_forward(s.banks()[a[0]], bank_name(s, a[0])), None
        if k == "filt_inv":
            return self.set_filters_inverse(s.banks()[a[0]]), None
        if k == "band_stats":
            return self.band_stats(), self.stats_slot
        if k == "estimate_sigma":
            return self.estimate_sigma(a[0]), self.sigma_slot
        if k == "select":
            return self.select(a[0], a[1]), self.sparsify_slot
        if k == "keep":
            rc = self.keep(a[0], a[1])
            return rc, (self.sparsify_slot if rc == 0 else None)
        if k == "threshold_bands":
            return self.threshold_bands(s.table(a[0]), a[1], a[2]), None
        if k == "denoise":
            rc = self.denoise(*a)
            return rc, ((self.sigma_slot, self.table_slot) if rc == 0 else None)
        if k == "read_band_stats":
            return 0, self.stats_slot
        if k == "read_sigma":
            return 0, self.sigma_slot
        if k == "last_thresholds":
            return 0, (self.sigma_slot, self.table_slot)
        if k == "last_sparsify":
            return 0, self.sparsify_slot
        if k == "take_band":
            return self.take_band(twin, a[0]), None
        raise ValueError(op)


def new_image(spec, seed):
    return spec.image(seed)


def new_band(spec, shape, seed):
    """values of both signs, the size of a detail band's"""
    return (oracle.hash_input(shape, seed, 60.0) - 30.0).astype(spec.dt)


def bank_name(spec, bank):
    return spec.wname if (bank == 0 and not spec.custom and spec.separable) else "custom"


def refused(op, rc):
    """Did the library (the model) turn the call down?"""
    k = op[0]
    if k in ("get_coeff", "get_coeff_at", "get_region"):
        return rc == 0
    if k in ("get_image", "get_image_at"):
        return rc <= 0
    return rc != 0


# --------------------------------------------------------------------------------------------------------------- the generator
class Situation(object):
    """The table of lazy_state.hpp (what plan.cpp's settle() performs) restated: what a deferring plan (can_defer_soft: separable
    2D SWT) would hold after each call.
    Tracked for every plan, deferring or not, so that all of them get the same kind of sequences."""

    def __init__(self):
        self.state, self.pending, self.consumed = FORWARD, False, False
        # have the details possibly been zeroed since the last forward()?  Then the noise estimate may be 0 and a BayesShrink entry
        # 0 / 0, which the table rule does not define: the generator gives such a denoise its noise level.  (No old kind asks.)
        # ... `flat`: the image is the reconstruction of such coefficients, and its transform has them again
        self.dead = self.flat = False
        self.spec = None   # the generator's plan: without one every keep counts as zeroing

    def name(self):
        return "pending" if self.pending else ("consumed" if self.consumed else "neither")

    def would_refuse(self, kind, custom_name):
        inv = self.state == INVERSE
        if kind in ("soft", "hard", "group", "shrink", "linf", "soft_norms", "get_coeff", "get_coeff_at", "get_region", "inverse"):
            return inv
        if kind in BAND_SWEEP:
            return inv
        if kind in ("add_dst", "add_src"):
            return inv or custom_name
        return False

    def step(self, op, custom_name):
        k = op[0]
        if self.would_refuse(k, custom_name):
            return
        if k in ("soft", "hard", "group", "soft_norms", "shrink") and len(op) > 1 and (op[1] >= BETAS["above"] or (k == "shrink" and op[1] == 0.0)):
            self.dead = True
        if k == "keep" and (self.spec is None or len(op) < 3 or min(np.atleast_1d(op[1])) < self.spec.swept_count(op[2]) - 1):
            self.dead = True   # (K >= N - 1 zeroes one value at the most)
        if k == "denoise" and (len(op) < 4 or op[3] is None):
            # the estimate of a white-noise image makes m - var cancel: thresholds of var / sqrt(eps).  A given noise level (at most
            # 9.0, against details of tens) leaves every band most of its values
            self.dead = True
        if k == "forward":
            self.state, self.pending, self.consumed, self.dead = FORWARD, False, False, self.flat
        elif k == "inverse":
            self.flat = self.dead
            self.state, self.consumed, self.pending = INVERSE, self.pending, False
        elif k in ("soft", "soft_norms"):
            beta, do_app = op[1], op[2]
            self.pending = (not do_app) and beta >= 0   # plan.cpp, defers(): `!do_app && beta >= 0 && can_defer_soft(p)`
        elif k in ("hard", "group", "shrink", "linf", "get_coeff", "get_coeff_at", "get_region", "add_dst", "add_src"):
            self.pending = False                         # Pending::apply
        elif k in ("norm1", "norm2sq", "norms_async"):
            self.pending = self.consumed = False         # the sums are over what a reader would see
        elif k in ("raw_read", "clone"):
            self.pending = self.consumed = False         # Pending::apply + Consumed::write_back
        elif k == "set_image":
            self.flat = False
            self.consumed = False                        # Consumed::write_back; a pending threshold stays pending
            self.state = INIT
        elif k in ("set_coeff", "take_band"):
            if k == "set_coeff" and self.spec is not None and op[1] == adaptive_ref.noise_band(self.spec.ndim):
                self.dead = False   # the noise band has values again: the estimate is not 0, and no table entry 0 / 0
            self.pending = self.consumed = False
            if op[1] == 0 and self.state == INVERSE:
                self.state = FORWARD
        elif k in READ_STATS:
            self.pending = self.consumed = False         # Pending::apply + Consumed::write_back, as the norms
        elif k in BAND_SWEEP:
            self.pending = False                         # Pending::apply


def generate(spec, seed, length=LENGTH, kinds=KINDS, count=None, shared_workspace=False):
    """`length` calls on a plan that has just run its first forward().  Steered, not uniform: the next call is the kind that this
    sequence has used least in the current lazy situation, and the sequence keeps moving through the three situations; refusals
    are capped and at least three forward() and three inverse() run.  Deterministic in (plan, seed).  `count`: a table of
    (situation, kind) -> uses shared by several sequences (see sequences()), so that together they cover every pair."""
    names = [p.name for p in PLANS]
    plan_index = names.index(spec.name) if spec.name in names else 99
    rng = np.random.default_rng([seed, plan_index, 20241])
    kinds = [k for k in kinds if not (k in ("filt_fwd", "filt_inv") and spec.hlen <= 2)]  # the 2-tap plans keep their bank
    sit = Situation()
    sit.spec = spec
    if count is None:
        count = {}
    for s in SITUATIONS:
        for k in kinds:
            count.setdefault((s, k), 0)
    ops, refusals, custom_name = [], 0, False
    ran = {"forward": 0, "inverse": 0}
    max_refusals = length // 5  # 20 %: the condition is 25 %
    nseed = [1000 * seed + 17]

    def fresh():
        nseed[0] += 1
        return nseed[0]

    def make(kind):
        cls = str(rng.choice(list(BETAS), p=[0.15, 0.15, 0.4, 0.1, 0.2]))
        beta = BETAS[cls]
        do_app, norm = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        if kind in ("soft", "soft_norms"):
            # the call that makes a threshold pending is do_app = 0 with beta >= 0: two calls in three
            if rng.random() < 0.67:
                do_app = 0
                if beta < 0:
                    beta = BETAS["inside"]
            return (kind, beta, do_app, norm)
        if kind == "hard":
            return (kind, beta, do_app, norm)
        if kind == "group":
            return (kind, beta, do_app if spec.swt else 0, norm)  # the approximation has the details' shape for the SWT only
        if kind == "shrink":
            return (kind, float(rng.choice(SHRINK_BETAS)), do_app)
        if kind == "linf":
            return (kind, abs(beta) if beta else 5.0, do_app)
        if kind in ("add_dst", "add_src"):
            return (kind, float(rng.choice([0.5, -1.25, 1.0])))
        if kind in ("get_image_at",):
            return (kind, int(rng.integers(0, spec.batch)))
        if kind == "get_coeff":
            return (kind, int(rng.integers(0, spec.nbands)))
        if kind == "get_coeff_at":
            return (kind, int(rng.integers(0, spec.nbands)), int(rng.integers(0, spec.batch)))
        if kind == "set_image":
            return (kind, fresh(), int(rng.integers(0, 2)))   # (seed of the new image, in place through pdwt_image_ptr)
        if kind == "set_coeff":
            # band 0 half of the time after an inverse (it re-arms the inverse), any band otherwise
            num = 0 if (sit.state == INVERSE and rng.random() < 0.5) else int(rng.integers(0, spec.nbands))
            return (kind, num, fresh(), int(rng.integers(0, 2)))
        if kind == "circshift":
            return (kind, int(rng.integers(-70, 70)), int(rng.integers(-70, 70)), int(rng.integers(0, 2)))
        if kind in ("filt_fwd", "filt_inv"):
            return (kind, int(rng.integers(0, 3)))
        if kind == "estimate_sigma":
            return (kind, do_app)   # (skip_zeros)
        if kind in ("select", "keep"):
            # K out of {0, 1, N/4, N-1, N, N+5} of the swept count; on a batched plan one K per image half of the time
            n = spec.swept_count(do_app)
            ks = (0, 1, n // 4, n - 1, n, n + 5)
            if spec.batch > 1 and norm:
                return (kind, tuple(int(ks[i]) for i in rng.integers(0, len(ks), spec.batch)), do_app)
            return (kind, int(ks[int(rng.integers(0, len(ks)))]), do_app)
        if kind == "threshold_bands":
            return (kind, fresh(), "hard" if norm else "soft", do_app)   # (seed of the table, op, the table is in device memory)
        if kind == "denoise":
            # the estimate (two in four; where the details may be zero the main loop sets the noise band first), one noise level, one
            # per image
            given = max(0, int(rng.integers(0, 4)) - 1)
            sigma = None if given == 0 else (GIVEN_SIGMA if given == 1 else tuple(3.0 + i % 7 for i in range(spec.batch)))
            return (kind, "VisuShrink" if norm else "BayesShrink", str(rng.choice(["soft", "hard"])), sigma, do_app)
        if kind == "take_band":
            return (kind, 0 if (sit.state == INVERSE and rng.random() < 0.5) else int(rng.integers(0, spec.nbands)))
        return (kind,)

    def emit(op):
        nonlocal refusals, custom_name
        k = op[0]
        if sit.would_refuse(k, custom_name):
            refusals += 1
        elif k in ran:
            ran[k] += 1
        count[(sit.name(), k)] += 1
        sit.step(op, custom_name)
        if k == "filt_fwd":
            custom_name = bank_name(spec, op[1]) != bank_name(spec, 0)
        ops.append(op)

    while len(ops) < length:
        left = length - len(ops)
        owed = max(0, 3 - ran["forward"]) + max(0, 3 - ran["inverse"])
        if shared_workspace and len(ops) >= 8 and sit.state != INVERSE and left > owed + 10:
            # once per sequence: the noise estimate and the K-term select share the radix-select workspace (both orders, nothing in
            # between), then three host uploads through the one pinned buffer back to back: a table, noise levels, K
            shared_workspace = False
            n = spec.swept_count(0)
            for op in (("estimate_sigma", 1), ("keep", n // 4, 0), ("estimate_sigma", 0), ("select", n - 1, 0),
                       ("threshold_bands", fresh(), "soft", 0), ("denoise", "VisuShrink", "hard", tuple(3.0 + i % 7 for i in range(spec.batch)) if spec.batch > 1 else GIVEN_SIGMA, 1),
                       ("keep", tuple(int(n // (2 + i % 3)) for i in range(spec.batch)) if spec.batch > 1 else n // 2, 1),
                       # ... and the whole recipe behind them, on a noise band with values
                       ("set_coeff", adaptive_ref.noise_band(spec.ndim), fresh(), 0), ("denoise", ("BayesShrink", "VisuShrink")[plan_index % 2], "soft", None, plan_index // 2 % 2)):
                emit(op)
            continue
        if owed and left <= owed + 2:  # the closing rounds
            emit(("forward",) if (sit.state == INVERSE or ran["inverse"] >= 3) else ("inverse",))
            continue
        # head for the situation this sequence has seen least
        seen = {s: sum(count[(s, k)] for k in kinds) for s in SITUATIONS}
        target = min(SITUATIONS, key=lambda s: (seen[s], rng.random()))
        here = sit.name()
        if target != here and rng.random() < 0.8:
            if target == "pending":
                emit(("forward",) if sit.state == INVERSE else ("soft", BETAS[str(rng.choice(["zero", "below", "inside", "above"], p=[0.15, 0.15, 0.6, 0.1]))], 0, int(rng.integers(0, 2))))
                continue
            if target == "consumed" and here == "pending":
                emit(("inverse",))
                continue
            if target == "neither" and sit.state == INVERSE:
                emit(make(str(rng.choice(["forward", "set_image", "set_coeff"]))))
                continue
        allowed = [k for k in kinds if refusals < max_refusals or not sit.would_refuse(k, custom_name)]
        least = min(count[(here, k)] for k in allowed)
        op = make(str(rng.choice([k for k in allowed if count[(here, k)] == least])))
        if op[0] == "denoise" and op[3] is None and sit.dead and left < 2:
            op = op[:3] + (GIVEN_SIGMA,) + op[4:]
        if op[0] == "denoise" and op[3] is None and sit.dead:
            emit(("set_coeff", adaptive_ref.noise_band(spec.ndim), fresh(), 0))   # the estimate needs a noise band that is not zero
        emit(op)
    return ops


_SEQUENCES = {}


def sequences():
    """{(plan name, seed): ops} of every sequence the GPU test runs: SEEDS through the C ABI with every kind, CLASS_SEED with the
    reference's methods.  Generated in one fixed order with one usage table for the plans that defer and one for the others, so
    that the least-used (situation, kind) pair anywhere is what the next sequence tries first."""
    if not _SEQUENCES:
        tables = {}
        for spec in PLANS:
            for seed in SEEDS + (CLASS_SEED,):
                kinds = REFERENCE_KINDS if seed == CLASS_SEED else KINDS
                _SEQUENCES[(spec.name, seed)] = generate(spec, seed, kinds=kinds, count=tables.setdefault((spec.defers, seed == CLASS_SEED), {}))
        # the seeds that also draw the adaptive and K-term calls: a pass and usage tables of their own, so that the ones above stay
        # byte for byte what they were (tests/test_plan_model_cpu.py holds their digest)
        tables = {}
        for spec in PLANS:
            for seed in NEW_SEEDS + (CLASS_SEED_2,):
                kinds = CLASS_KINDS if seed == CLASS_SEED_2 else ALL_KINDS
                # (the old kinds start three uses ahead in every situation: the new ones get there first)
                table = tables.setdefault((spec.defers, seed == CLASS_SEED_2), {(s, k): 3 for s in SITUATIONS for k in KINDS})
                _SEQUENCES[(spec.name, seed)] = generate(spec.single() if seed == CLASS_SEED_2 else spec, seed, kinds=kinds, count=table,
                                                         shared_workspace=seed == NEW_SEEDS[-1])
    return _SEQUENCES


def as_python(spec, seed, ops, upto=None):
    """The call list as runnable Python (what a failing sequence prints)."""
    lines = ["from plan_model import PLANS", "from test_gpu_sequences import run_ops",
             "spec = [p for p in PLANS if p.name == %r][0]" % spec.name, "ops = ["]
    lines += ["    %r," % (op,) for op in (ops if upto is None else ops[:upto + 1])]
    lines += ["]", "run_ops(spec, ops)  # generated with seed %d" % seed]
    return "\n".join(lines)
