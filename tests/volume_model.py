"""An EAGER host model of one volume handle of include/pypwt_amd.h (pdwt_volume_*: `Wavelets3D` / `Wavelets3D64`, decimated and
stationary), the generator of the call sequences it judges, and the comparator that drives a handle and the model with the same
calls.  numpy only: no GPU, no ctypes.

The library's handle carries a good deal across calls (pypwt_amd/csrc/volume.cpp): one batched 2D plan per level with a state
machine of its own, a radix-select workspace and a pinned staging buffer that several operators share, the accumulated shift of
a cycle-spinning volume, the level-1 stack as scratch of the circular shifts, two extra volumes of cycle_spin, and the hidden
intermediates A_1 .. A_{L-1}.  The model has none of that: an image, the 1 + 7 L sub-bands, a state, a shift and the result slots;
every call takes effect at once, a refused call changes nothing and returns the library's code.  So whatever the library returns
after ANY order of calls has one right answer here.

Every operation is the composition of references the suite already has and pins elsewhere -- nothing is derived again:
  volume_ref / volume_swt_ref      forward, inverse, soft / hard threshold (tests/golden/volume.npz, volume_swt.npz pin them to pywt)
  volume_prox_ref                  group_soft, group_norm, linf, shrink, axpy
  volume_ops_ref                   band_stats, estimate_sigma, threshold_table, threshold_bands, select_magnitude, keep_largest
  volume_spin_ref                  shift, cycle_spin

What every entry point owes the state is the table of docs/KERNELS.md ("What every volume entry point owes the state"), restated
by `VolumeState.refusal` / `VolumeState.advance` below and read off include/pypwt_amd.h and volume.cpp:

  forward            0 in every state; a cycle-spinning volume first shifts the image by a fresh draw (three of splitmix64, one per
                     axis, each modulo the axis) and ADDS the draw to its shift; state FORWARD
  inverse            PDWT_ERR_STATE in state INVERSE, nothing done; else state INVERSE, the coefficients are NOT modified; a
                     cycle-spinning volume shifts the result back by the whole shift, which becomes zero
  soft / hard / group / linf / shrink, norms, group_norm
                     PDWT_ERR_STATE in state INVERSE, nothing done; the state does not change
  add_wavelet        PDWT_ERR_STATE when either operand is in state INVERSE
  get_image          the element count, every state;  get_coeff  0 values in state INVERSE (the buffer is not written)
  raw read           pdwt_volume_coeff_ptr + pdwt_volume_read: legal in every state
  set_image          state INIT, the shift becomes zero;  set_coeff  num 0 in state INVERSE re-arms: state FORWARD
  circshift          PDWT_ERR_STATE in state FORWARD (the image is not current); else the image is rolled, state INIT, the shift stays
  set_cycle_spinning on: PDWT_ERR_UNSUPPORTED for a stationary volume, else the generator restarts from the seed;
                     off: PDWT_ERR_STATE while the image is shifted
  cycle_spin         stationary: PDWT_ERR_UNSUPPORTED; state FORWARD or cycle spinning on: PDWT_ERR_STATE; else the mean over the
                     shifts becomes the image, the coefficients are those of the LAST shift after its threshold, state INVERSE
  band_stats, estimate_sigma, select_magnitude, norms_async (read only), threshold_bands, denoise, keep_largest (sweeps)
                     stationary: PDWT_ERR_UNSUPPORTED; PDWT_ERR_STATE in state INVERSE; the state does not change
  the result slots   (adaptive_slots, sparsify_slots + pdwt_volume_read) stationary: PDWT_ERR_UNSUPPORTED; else every state; a slot
                     nothing has written yet reads as zeros (the workspace is zeroed when it is allocated)
"""
import json
import os

import numpy as np

import ops_ref
import volume_ops_ref
import volume_prox_ref
import volume_ref
import volume_spin_ref
import volume_swt_ref

INIT, FORWARD, INVERSE = 0, 1, 2
STATES = (INIT, FORWARD, INVERSE)
STATE_NAMES = {INIT: "INIT", FORWARD: "FORWARD", INVERSE: "INVERSE"}
OK, ERR_STATE, ERR_UNSUPPORTED = 0, -4, -7
U53 = 2.0 ** -53

KINDS = ("forward", "inverse", "soft", "hard", "group", "linf", "shrink", "norms", "group_norm", "add_dst", "add_src",
         "get_image", "get_coeff", "raw_read", "set_image", "set_coeff", "circshift", "spin_on", "spin_off", "current_shift",
         "cycle_spin", "band_stats", "estimate_sigma", "threshold_bands", "denoise", "select", "keep", "norms_async",
         "read_sigma", "read_band_stats", "read_norms", "last_thresholds", "last_sparsify")
# ... and the ones `Wavelets3D` has a method for (all but the raw read through pdwt_volume_coeff_ptr, which is image_device's business)
CLASS_KINDS = tuple(k for k in KINDS if k != "raw_read")
READERS = ("read_sigma", "read_band_stats", "read_norms", "last_thresholds", "last_sparsify")
DWT_ONLY = ("band_stats", "estimate_sigma", "threshold_bands", "denoise", "select", "keep", "norms_async") + READERS
NEEDS_COEFFS = ("inverse", "soft", "hard", "group", "linf", "shrink", "norms", "group_norm", "band_stats", "estimate_sigma",
                "threshold_bands", "denoise", "select", "keep", "norms_async")
SELECTS = ("select", "keep")

# beta classes on volumes of 0..255: zero, below nearly every detail, inside their range, above all of them, negative
BETAS = {"zero": 0.0, "below": 1e-3, "inside": 40.0, "above": 1e6, "negative": -1.5}
SHRINK_BETAS = (0.25, 0.0, 3.0, -0.5)
SPIN_SIGMA = 17.25


class VolumeSpec(object):
    """One volume of the table below.  `levels` is what the library keeps after its clamp; `cycle`: 0, or the seed cycle spinning
    is turned on with before the first forward; `segments`: None, or the steps per depth segment forced on every level through
    the test hook pdwt_volume_set_depth_segments."""

    def __init__(self, name, shape, wname, levels, swt=0, prec="f32", cycle=0, segments=None):
        self.name, self.shape, self.wname, self.asked = name, tuple(shape), wname, levels
        self.swt, self.prec, self.cycle, self.segments = swt, prec, cycle, segments
        self.hlen = volume_ref.hlen_of(wname)
        self.levels = volume_ref.clamp_levels(self.shape, self.hlen, levels)
        self.dt = np.float64 if prec == "f64" else np.float32
        self.nbands = 1 + 7 * self.levels

    def __repr__(self):
        return self.name

    def band_shapes(self):
        return (volume_swt_ref if self.swt else volume_ref).band_shapes(self.shape, self.levels)

    def image(self, seed):
        """uniform(0, 255), the same for every precision (drawn in float32)"""
        rng = np.random.default_rng([int(seed), sum(self.shape), 3301])
        return rng.uniform(0.0, 255.0, self.shape).astype(np.float32).astype(self.dt)

    def band(self, num, seed):
        """values of both signs, the size of a detail sub-band's"""
        rng = np.random.default_rng([int(seed), num, 3307])
        return rng.uniform(-60.0, 60.0, self.band_shapes()[num]).astype(np.float32).astype(self.dt)

    def table(self, seed, app):
        """thresholds of threshold_bands: one NaN (left alone), one zero; entry 0 NaN unless `app` (tests/test_gpu_volume_ops.py)"""
        T = np.random.default_rng([int(seed), 3313]).uniform(0.5, 30.0, self.nbands).astype(self.dt)
        T[self.nbands - 2] = np.nan
        T[1] = 0.0
        if not app:
            T[0] = np.nan
        return T

    def swept(self, do_app):
        shapes = self.band_shapes()
        return sum(int(np.prod(s)) for s in shapes[0 if do_app else 1:])


VOLUMES = [
    # the shapes of tests/volume_spin_ref.py (db2 keeps ONE level on the first two: the level clamp)
    VolumeSpec("dwt-9x10x12-db2-L1", (9, 10, 12), "db2", 2),
    VolumeSpec("dwt-8x8x16-db2-L1", (8, 8, 16), "db2", 2),
    VolumeSpec("dwt-5x7x11-haar-L2", (5, 7, 11), "haar", 2),
    # tests/test_gpu_volume.py: odd depth, P % 4 = 2.  Its CASES hold no depth below the filter length; the stationary suite's
    # (tests/test_gpu_volume_swt.py) does: 4 slices under 40 taps
    VolumeSpec("dwt-9x10x13-db2-L1", (9, 10, 13), "db2", 1),
    VolumeSpec("swt-4x40x44-db20-L1", (4, 40, 44), "db20", 1, swt=1),
    # ... and decimated: shape B of tests/test_gpu_volume_taps.py, 7 slices under 8 taps (the source counter of the depth pass wraps)
    VolumeSpec("dwt-7x9x11-db4-L1", (7, 9, 11), "db4", 1),
    # several depth segments per walk: 1 step (level 1 walks 3 steps forward, level 2 two), 3 steps (of 4)
    VolumeSpec("dwt-5x7x11-haar-L2-seg1", (5, 7, 11), "haar", 2, segments=1),
    VolumeSpec("dwt-8x8x16-db2-L1-seg3", (8, 8, 16), "db2", 2, segments=3),
    # stationary, two levels: dilation 2 does not divide the depth of 5
    VolumeSpec("swt-5x7x11-haar-L2", (5, 7, 11), "haar", 2, swt=1),
    VolumeSpec("swt-8x8x16-haar-L2", (8, 8, 16), "haar", 2, swt=1),
    VolumeSpec("dwt-5x7x11-haar-L2-f64", (5, 7, 11), "haar", 2, prec="f64"),
    VolumeSpec("swt-5x7x11-haar-L2-f64", (5, 7, 11), "haar", 2, swt=1, prec="f64"),
    VolumeSpec("dwt-9x10x12-db2-L1-cycle", (9, 10, 12), "db2", 2, cycle=11),
    VolumeSpec("dwt-5x7x11-haar-L2-cycle", (5, 7, 11), "haar", 2, cycle=12),
]
SEEDS = (1, 2, 3, 4)   # the C-ABI sequences of every volume
CLASS_SEED = 5         # the one through the Python class
LENGTH = 40


def spec_named(name):
    return [s for s in VOLUMES if s.name == name][0]


def splitmix64(state):
    """(new state, draw): volume.cpp, spin_draw"""
    m = (1 << 64) - 1
    state = (state + 0x9E3779B97F4A7C15) & m
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return state, z ^ (z >> 31)


# ------------------------------------------------------------------------------------------------- what the state machine owes
class VolumeState(object):
    """The part of a handle that decides what is refused: state, cycle spinning, its generator and the shift.  The generator of
    the sequences tracks this alone; the model adds the data."""

    def __init__(self, spec):
        self.spec = spec
        self.state = INIT
        self.spinning = False
        self.rng = 0
        self.shift = (0, 0, 0)
        self.after_select = False  # the last call that used the radix-select workspace was select / keep (coverage only)

    def refusal(self, op, twin_state=FORWARD):
        """The code the library turns `op` down with in this state (0 for get_coeff: "0 values"), or None when it runs."""
        k = op[0]
        if self.spec.swt and (k in DWT_ONLY or k == "spin_on" or k == "cycle_spin"):
            return ERR_UNSUPPORTED
        if k == "cycle_spin" and (self.state == FORWARD or self.spinning):
            return ERR_STATE
        if k == "spin_off" and self.spinning and any(self.shift):
            return ERR_STATE
        if k == "circshift" and self.state == FORWARD:
            return ERR_STATE
        if k in NEEDS_COEFFS and self.state == INVERSE:
            return ERR_STATE
        if k in ("add_dst", "add_src") and INVERSE in (self.state, twin_state):
            return ERR_STATE
        if k == "get_coeff" and self.state == INVERSE:
            return 0
        return None

    def draw(self):
        d = []
        for n in self.spec.shape:
            self.rng, z = splitmix64(self.rng)
            d.append(int(z % n))
        return tuple(d)

    def advance(self, op):
        """State, shift and generator after an ACCEPTED `op`; returns the draw of a spinning forward (else None)."""
        k = op[0]
        d = None
        if k == "forward":
            if self.spinning:
                d = self.draw()
                self.shift = self.accumulate(d)
            self.state = FORWARD
        elif k == "inverse":
            self.state = INVERSE
            if self.spinning:
                self.shift = (0, 0, 0)
        elif k == "set_image":
            self.state = INIT
            self.shift = self.shift_after_set_image()
        elif k == "set_coeff":
            if op[1] == 0 and self.state == INVERSE:
                self.state = self.state_after_rearm()
        elif k == "circshift":
            self.state = self.state_after_circshift()
        elif k == "spin_on":
            self.spinning, self.rng = True, int(op[1])
        elif k == "spin_off":
            self.spinning, self.rng = False, 0
        elif k == "cycle_spin":
            self.state = self.state_after_cycle_spin()
        if k in SELECTS:
            self.after_select = True
        elif k in ("estimate_sigma",) or (k == "denoise" and op[3] is None):
            self.after_select = False
        return d

    # (what the planted defects of tests/test_volume_model_cpu.py replace)
    def accumulate(self, d):
        return tuple((s + x) % n for s, x, n in zip(self.shift, d, self.spec.shape))

    def shift_after_set_image(self):
        return (0, 0, 0)

    def state_after_rearm(self):
        return FORWARD

    def state_after_circshift(self):
        return INIT

    def state_after_cycle_spin(self):
        return INVERSE


# --------------------------------------------------------------------------------------------------------------- the model
class VolumeModel(VolumeState):
    def __init__(self, spec, image):
        VolumeState.__init__(self, spec)
        self.image = np.array(image, dtype=spec.dt).reshape(spec.shape)
        self.bands = [np.zeros(s, dtype=spec.dt) for s in spec.band_shapes()]  # never computed: zeros, like a plan's arena
        # the result slots: zeros until something writes them
        self.sigma = np.zeros(1, np.float64)
        self.table = np.zeros(spec.nbands, spec.dt)
        self.stats = np.zeros((spec.nbands, 2), np.float64)
        self.norms_slot = np.zeros(2, np.float64)
        self.sparsify = (np.zeros(1, spec.dt), np.zeros(1, np.uint64))

    # ---- arithmetic: the references
    def _double(self, double=None):
        return ("full" if self.spec.prec == "f64" else False) if double is None else double

    def transform(self, image, double=None):
        s = self.spec
        if s.swt:
            out = volume_swt_ref.forward(image, s.wname, s.levels, self._double(double))
        else:
            out = volume_ref.forward(image, s.wname, s.levels, self._double(double))
        return [np.ascontiguousarray(b) for b in out]

    def reconstruct(self, bands, double=None):
        s = self.spec
        if s.swt:
            return np.ascontiguousarray(volume_swt_ref.inverse(bands, s.wname, s.levels, self._double(double)))
        return np.ascontiguousarray(volume_ref.inverse(bands, s.shape, s.wname, s.levels, self._double(double)))

    def _global(self, bands, mode, beta, do_app, normalize):
        ref = volume_swt_ref if self.spec.swt else volume_ref
        return ref.threshold(bands, self.spec.levels, mode, beta, do_app, normalize)

    def exact_norms(self):
        return ops_ref.norms(self.bands)

    # ---- the calls
    def forward(self):
        d = self.advance(("forward",))
        if d is not None:
            self.image = volume_spin_ref.shift(self.image, d)
        self.bands = self.transform(self.image)
        return OK

    def inverse(self):
        shift = self.shift
        self.advance(("inverse",))
        self.image = self.reconstruct(self.bands)
        if self.spinning:
            self.image = volume_spin_ref.shift(self.image, [-v for v in shift])
        return OK

    def threshold(self, mode, beta, do_app, normalize):
        self.bands = self._global(self.bands, mode, beta, do_app, normalize)
        return OK

    def group(self, beta, do_app, normalize):
        self.bands = volume_prox_ref.group_soft(self.bands, self.spec.levels, beta, do_app, normalize)
        return OK

    def linf(self, beta, do_app):
        self.bands = volume_prox_ref.linf(self.bands, beta, do_app)
        return OK

    def shrink(self, beta, do_app):
        self.bands = volume_prox_ref.shrink(self.bands, beta, do_app)
        return OK

    def add_wavelet(self, src, alpha):
        """self += alpha * src"""
        self.bands = volume_prox_ref.axpy(self.bands, src.bands, alpha)
        return OK

    def cycle_spin(self, variant, mode, value, do_app, normalize, nshifts):
        """value: the global beta ("global") or the given noise level ("visu"); the lattice's first `nshifts` shifts"""
        s = self.spec
        shifts = volume_spin_ref.lattice(nshifts)
        kw = dict(mode=mode, beta=value, do_app=do_app, normalize=normalize) if variant == "global" else \
            dict(mode=mode, method="VisuShrink", sigma=value)
        x = self.image
        self.image = np.ascontiguousarray(volume_spin_ref.cycle_spin(x, s.wname, s.levels, shifts, double=self._double(), **kw))
        # the coefficients left behind: the last shift's, after its threshold
        last = self.transform(volume_spin_ref.shift(x, shifts[-1]))
        if variant == "global":
            self.bands = self._global(last, mode, value, do_app, normalize)
        else:
            self.sigma, self.table, self.bands = volume_ops_ref.denoise(last, s.shape, "VisuShrink", mode, value)
        self.advance(("cycle_spin",))
        return OK

    def denoise(self, method, mode, sigma, skip):
        if method == "BayesShrink":
            self.stats = volume_ops_ref.band_stats(self.bands)
        self.sigma, self.table, self.bands = volume_ops_ref.denoise(self.bands, self.spec.shape, method, mode, sigma, skip)
        return OK

    def estimate_sigma(self, skip):
        self.sigma = volume_ops_ref.estimate_sigma(self.bands, skip)
        return OK

    def select(self, k, do_app):
        self.sparsify = volume_ops_ref.select_magnitude(self.bands, k, do_app)
        return OK

    def keep(self, k, do_app):
        thr, kept, self.bands = volume_ops_ref.keep_largest(self.bands, k, do_app)
        self.sparsify = (thr, kept)
        return OK

    # ---- one op of a generated sequence
    def apply(self, op, twin=None):
        """(return value, what the call hands the host or None).  A refused call changes nothing."""
        k, a = op[0], op[1:]
        s = self.spec
        rc = self.refusal(op, twin.state if twin is not None else FORWARD)
        if rc is not None:
            return rc, None
        if k == "forward":
            return self.forward(), None
        if k == "inverse":
            return self.inverse(), None
        if k in ("soft", "hard"):
            return self.threshold(k, *a), None
        if k == "group":
            return self.group(*a), None
        if k == "linf":
            return self.linf(*a), None
        if k == "shrink":
            return self.shrink(*a), None
        if k == "norms":
            return OK, self.exact_norms()
        if k == "group_norm":
            return OK, float(volume_prox_ref.group_norm(self.bands, s.levels, a[0]))
        if k == "add_dst":
            return self.add_wavelet(twin, a[0]), None
        if k == "add_src":
            return twin.add_wavelet(self, a[0]), None
        if k == "get_image":
            return self.image.size, self.image
        if k == "get_coeff":
            return self.bands[a[0]].size, self.bands[a[0]]
        if k == "raw_read":
            return OK, self.bands
        if k == "set_image":
            self.image = s.image(a[0])
            self.advance(op)
            return OK, None
        if k == "set_coeff":
            self.bands = list(self.bands)
            self.bands[a[0]] = s.band(a[0], a[1])
            self.advance(op)
            return OK, None
        if k == "circshift":
            self.image = volume_spin_ref.shift(self.image, a[:3])
            self.advance(op)
            return OK, None
        if k in ("spin_on", "spin_off"):
            self.advance(op)
            return OK, None
        if k == "current_shift":
            return OK, self.shift
        if k == "cycle_spin":
            return self.cycle_spin(*a), None
        if k == "band_stats":
            self.stats = volume_ops_ref.band_stats(self.bands)
            return OK, self.stats
        if k == "estimate_sigma":
            rc = self.estimate_sigma(a[0])
            self.advance(op)
            return rc, self.sigma
        if k == "threshold_bands":
            self.bands = volume_ops_ref.threshold_bands(self.bands, s.table(a[0], a[2]), a[1])
            return OK, None
        if k == "denoise":
            rc = self.denoise(*a)
            self.advance(op)
            return rc, (self.sigma, self.table)
        if k == "select":
            rc = self.select(*a)
            self.advance(op)
            return rc, self.sparsify
        if k == "keep":
            rc = self.keep(*a)
            self.advance(op)
            return rc, self.sparsify
        if k == "norms_async":
            self.stats = volume_ops_ref.band_stats(self.bands)
            self.norms_slot = np.array(self.exact_norms(), dtype=np.float64)
            return OK, self.norms_slot
        if k == "read_sigma":
            return OK, self.sigma
        if k == "read_band_stats":
            return OK, self.stats
        if k == "read_norms":
            return OK, self.norms_slot
        if k == "last_thresholds":
            return OK, (self.sigma, self.table)
        if k == "last_sparsify":
            return OK, self.sparsify
        raise ValueError(op)


def refused(op, rc):
    """Did the library (the model) turn the call down?"""
    if op[0] == "get_coeff":
        return rc == 0
    if op[0] == "get_image":
        return rc <= 0
    return rc != 0


# ------------------------------------------------------------------------------------- the recorded refusals (tests/golden)
# label of tests/test_gpu_volume_refusals.py's walk -> the op it is here
_RECORDED = {
    "inverse": ("inverse",), "get_coeff": ("get_coeff", 1), "soft_threshold": ("soft", 1.0, 0, 0), "hard_threshold": ("hard", 1.0, 0, 0),
    "norms": ("norms",), "band_stats_async": ("band_stats",), "norms_async": ("norms_async",), "estimate_sigma_async": ("estimate_sigma", 1),
    "threshold_bands": ("threshold_bands", 1, "soft", 1), "denoise_async": ("denoise", "BayesShrink", "soft", 1.0, 1),
    "adaptive_slots": ("read_sigma",), "select_magnitude_async": ("select", 3, 0), "keep_largest_async": ("keep", 3, 0),
    "sparsify_slots": ("last_sparsify",), "set_coeff num=1": ("set_coeff", 1, 1, 0), "set_coeff num=0": ("set_coeff", 0, 1, 0),
}


def recorded_refusals(path=None):
    """[(walk key, label, state the call is made in, op, recorded code)] of every entry of tests/golden/volume_refusals.json that
    this model has an op for: the operators after forward(), everything after inverse(), and what set_coeff(0) restores."""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volume_refusals.json")
    with open(path) as f:
        walks = json.load(f)["walks"]
    out = []
    for key, walk in sorted(walks.items()):
        for label, value, _ in walk:
            if label.startswith("after inverse: "):
                state, name = INVERSE, label[len("after inverse: "):]
            elif label.startswith("restored: "):
                state, name = FORWARD, label[len("restored: "):]
            elif label in _RECORDED and label not in ("inverse",):
                state, name = FORWARD, label
            else:
                continue
            if name in _RECORDED and not isinstance(value, list):
                out.append((key, label, state, _RECORDED[name], value))
    return out


# --------------------------------------------------------------------------------------------------------------- the generator
def covered_pairs(spec, ops_of_seeds):
    """{(state the call was made in, kind)} over sequences that each start after the first forward()"""
    seen = set()
    for ops in ops_of_seeds:
        st = start_state(spec)
        for op in ops:
            seen.add((st.state, op[0]))
            if st.refusal(op) is None:
                st.advance(op)
    return seen


def start_state(spec):
    """the tracker of a handle that has just run its first forward()"""
    st = VolumeState(spec)
    if spec.cycle:
        st.advance(("spin_on", spec.cycle))
    st.advance(("forward",))
    return st


# orderings every volume's sequences contain, whatever the steering does (seed -> ops opening that sequence)
def _openers(spec, seed):
    if seed == 1:  # the shared radix-select workspace: estimate, K-term, estimate again; two thresholds in a row with other betas
        return [("estimate_sigma", 1), ("keep", spec.swept(0) // 3, 0), ("estimate_sigma", 1), ("read_sigma",), ("soft", 40.0, 0, 0),
                ("hard", 12.0, 1, 1), ("group", 20.0, 0, 1)]
    if seed == 2:
        out = [("select", spec.swept(1) // 2, 1), ("estimate_sigma", 0), ("last_sparsify",), ("hard", 40.0, 0, 0), ("soft", 6.0, 0, 0),
               ("group", 30.0, 1, 0)]
        if spec.cycle:  # two forwards in a row, spin_off and set_image while shifted
            out += [("forward",), ("current_shift",), ("spin_off",), ("set_image", 2001, 0), ("current_shift",)]
        return out
    if seed == 3 and spec.cycle:  # circshift after inverse then a getter; cycle_spin while spinning is on
        return [("inverse",), ("circshift", 2, -3, 5), ("get_coeff", 1), ("cycle_spin", "global", "soft", 40.0, 0, 0, 2), ("forward",),
                ("forward",), ("inverse",)]
    if seed == 4 and spec.cycle:
        return [("forward",), ("set_image", 4001, 1), ("forward",), ("inverse",), ("spin_off",),
                ("cycle_spin", "visu", "soft", SPIN_SIGMA, 0, 0, 2)]
    if seed == CLASS_SEED:  # a threshold, an inverse and a forward that RUN, whatever the steering does with the refusals
        return [("soft", 40.0, 0, 1), ("inverse",), ("get_image",), ("forward",), ("hard", 12.0, 1, 0)]
    return []


def generate(spec, seed, length=LENGTH, kinds=KINDS, seen=None, per_state=True):
    """`length` calls on a handle that has just run its first forward().  Steered, not uniform: the next call is a kind this
    volume's sequences have not yet made in the current state; when the state has none left the sequence moves to the state that
    has most (`per_state` false: a kind it has not made at all).  Deterministic in (volume, seed).  `seen`: the (state, kind) pairs of the volume's earlier sequences (see sequences())."""
    rng = np.random.default_rng([seed, VOLUMES.index(spec) if spec in VOLUMES else 99, 20251])
    seen = set() if seen is None else seen
    st = start_state(spec)
    ops = []
    nseed = [1000 * seed + 17]
    flip = {}

    def fresh():
        nseed[0] += 1
        return nseed[0]

    def alternate(key):
        flip[key] = 1 - flip.get(key, int(rng.integers(0, 2)))
        return flip[key]

    def make(kind):
        cls = str(rng.choice(list(BETAS), p=[0.1, 0.2, 0.5, 0.05, 0.15]))
        beta = BETAS[cls]
        if kind in ("soft", "hard"):
            return (kind, beta, int(rng.integers(0, 2)), int(rng.integers(0, 2)))
        if kind == "group":
            return (kind, abs(beta), alternate("group"), int(rng.integers(0, 2)))
        if kind == "linf":
            return (kind, abs(beta) if beta else 5.0, int(rng.integers(0, 2)))
        if kind == "shrink":
            return (kind, float(rng.choice(SHRINK_BETAS)), int(rng.integers(0, 2)))
        if kind == "group_norm":
            return (kind, int(rng.integers(0, 2)))
        if kind in ("add_dst", "add_src"):
            return (kind, float(rng.choice([0.5, -1.25, 1.0])))
        if kind == "get_coeff":
            return (kind, int(rng.integers(0, spec.nbands)))
        if kind == "set_image":
            return (kind, fresh(), alternate("set_image"))   # (seed of the new image, in place through pdwt_volume_image_ptr)
        if kind == "set_coeff":
            num = 0 if (st.state == INVERSE and rng.random() < 0.6) else int(rng.integers(0, spec.nbands))
            return (kind, num, fresh(), alternate("set_coeff"))
        if kind == "circshift":
            return (kind,) + tuple(int(v) for v in rng.integers(-20, 20, 3))
        if kind == "spin_on":
            return (kind, int(rng.integers(1, 1 << 40)))
        if kind == "cycle_spin":
            if alternate("cycle_spin"):
                return (kind, "global", str(rng.choice(["soft", "hard"])), 40.0, int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(1, 4)))
            return (kind, "visu", str(rng.choice(["soft", "hard"])), SPIN_SIGMA, 0, 0, int(rng.integers(1, 4)))
        if kind == "estimate_sigma":
            return (kind, int(rng.integers(0, 2)))
        if kind == "threshold_bands":
            return (kind, fresh(), str(rng.choice(["soft", "hard"])), int(rng.integers(0, 2)))
        if kind == "denoise":
            return (kind, str(rng.choice(["BayesShrink", "VisuShrink"])), str(rng.choice(["soft", "hard"])),
                    None if rng.random() < 0.6 else SPIN_SIGMA, int(rng.integers(0, 2)))
        if kind in SELECTS:
            do_app = int(rng.integers(0, 2))
            n = spec.swept(do_app)
            return (kind, int(rng.choice([0, 1, n // 10, n // 2, n, n + 5])), do_app)
        return (kind,)

    def emit(op):
        ran = st.refusal(op) is None
        if ran or op[0] != "cycle_spin" or spec.swt or st.state == FORWARD or (st.state, "tried") in seen:
            seen.add((st.state if per_state else None, op[0]))
        elif per_state:
            seen.add((st.state, "tried"))  # (once more at most: the sequence must not spend itself on one pair)
        if ran:
            st.advance(op)
            if op[0] == "cycle_spin":
                seen.add(("ran", op[1]))
        ops.append(op)

    def leaves(kind):
        """does an accepted call of `kind` (usually) leave the current state?"""
        return kind in {INIT: ("forward", "inverse", "cycle_spin"), FORWARD: ("inverse", "set_image"),
                        INVERSE: ("forward", "set_image", "set_coeff", "circshift")}[st.state]

    def head_for(target):
        if target == FORWARD:
            return ("forward",) if st.state == INIT or rng.random() < 0.5 else ("set_coeff", 0, fresh(), alternate("set_coeff"))
        if target == INVERSE:
            return ("inverse",)
        if st.state == INVERSE and rng.random() < 0.5:
            return make("circshift")
        return make("set_image")

    for op in _openers(spec, seed):
        if op[0] in kinds:
            emit(op)
    while len(ops) < length:
        # both variants of cycle_spin RUN on every decimated volume: it is refused while the volume draws shifts of its own
        owed = [v for v in ("global", "visu") if ("ran", v) not in seen] if ("cycle_spin" in kinds and not spec.swt) else []
        if owed and st.state != FORWARD and not any(st.shift) and len(ops) + 3 <= length:
            if st.spinning:
                emit(("spin_off",))
            flip["cycle_spin"] = 0 if owed[0] == "global" else 1
            emit(make("cycle_spin"))
            if spec.cycle:
                emit(make("spin_on"))
            continue
        missing = {s: [k for k in kinds if (s if per_state else None, k) not in seen] for s in STATES}
        here = missing[st.state]
        stay = [k for k in here if not leaves(k)]
        if stay or here:
            kind = str(rng.choice(stay or here))
            if kind == "cycle_spin" and st.spinning and not any(st.shift) and "spin_off" in kinds:
                emit(("spin_off",))  # so that it runs: it is refused while the volume draws shifts of its own
            emit(make(kind))
        elif any(missing.values()):
            emit(head_for(max(STATES, key=lambda s: (len(missing[s]), rng.random()))))
        else:
            emit(make(str(rng.choice(kinds))))
    return ops[:length]


_SEQUENCES = {}


def sequences():
    """{(volume name, seed): ops} of every sequence the GPU test runs: SEEDS through the C ABI with every kind, CLASS_SEED with the
    class's methods.  The seeds of a volume share one table of (state, kind) pairs, so that together they cover every pair."""
    if not _SEQUENCES:
        for spec in VOLUMES:
            seen = set()
            for seed in SEEDS:
                _SEQUENCES[(spec.name, seed)] = generate(spec, seed, seen=seen)
            _SEQUENCES[(spec.name, CLASS_SEED)] = generate(spec, CLASS_SEED, kinds=CLASS_KINDS, per_state=False)
    return _SEQUENCES


def as_python(spec, seed, ops, upto=None):
    """The call list as runnable Python (what a failing sequence prints)."""
    lines = ["from volume_model import spec_named", "from test_gpu_volume_sequences import run_ops",
             "spec = spec_named(%r)" % spec.name, "ops = ["]
    lines += ["    %r," % (op,) for op in (ops if upto is None else ops[:upto + 1])]
    lines += ["]", "run_ops(spec, ops, seed=%d)  # generated with seed %d" % (seed, seed)]
    return "\n".join(lines)


# --------------------------------------------------------------------------------------------------------------- the bounds
def transform_bound(spec, ref64, ref32):
    """tests/test_gpu_volume.py / test_gpu_volume_swt.py (tol32): the larger of the rule and twice the distance between the fp32
    and the fp64 composition -- measured on the reference pair, never on the library, so it scales with whatever data a sequence
    hands the volume; fp64: 1e-12 max(1, max |ref|)."""
    rmax = max(float(np.abs(ref64).max()), 1.0)
    if spec.prec == "f64":
        return 1e-12 * rmax
    return max(1.5e-6 * (1 + spec.levels) * rmax, 2.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()))


def group_bound(spec, ref_band):
    """tests/test_gpu_volume_prox.py: band_bound"""
    eps = 5e-6 if spec.prec == "f32" else 8 * 2.0 ** -52
    return eps * max(float(np.abs(ref_band).max()), 1.0)


def table_bounds(spec, bands, sigma, method):
    """tests/test_gpu_volume_ops.py, check_table: (the reference table, the relative bound of every entry -- inf where the rule
    leaves a sub-band out: within the sum bound of the max(., eps) edge).  Entry 0 is NaN in both.  A sub-band that a threshold has
    zeroed under a noise level of zero (m = var = 0) is not at that edge: the threshold is 0 / sqrt(eps) = 0 on both sides, and an
    entry whose reference is 0 is compared exactly whatever its bound."""
    dt = np.dtype(spec.dt)
    stats = volume_ops_ref.band_stats(bands)
    want = volume_ops_ref.threshold_table(bands, sigma, method, spec.shape, stats=stats)
    rounding = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    eps = float(np.finfo(dt).eps)
    bound = np.full(spec.nbands, np.inf)
    for num in range(1, spec.nbands):
        n = bands[num].size
        if method == "VisuShrink":
            bound[num] = 2 * rounding
            continue
        var = float(sigma[0]) * float(sigma[0])
        m = stats[num, 1] / n
        if abs(m - var - eps) < 2.0 * n * U53 * m:
            continue
        bound[num] = rounding + (m / abs(m - var) if m != var else 0.0) * n * 2.0 ** -52
    return want, bound


# --------------------------------------------------------------------------------------------------------------- the comparator
class Mismatch(AssertionError):
    pass


def _check(cond, msg, *args):
    if not cond:
        raise Mismatch(msg % args if args else msg)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    _check(got.dtype == want.dtype and got.size == want.size, "%s: %s of %d values, the model has %s of %d", what, got.dtype, got.size,
           want.dtype, want.size)
    g, w = got.reshape(-1), want.reshape(-1)
    if not ops_ref.same_bits(g, w):
        bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))) | (np.signbit(g) != np.signbit(w)))
        raise Mismatch("%s: %d of %d values differ from the model, first at %d: %r != %r" % (what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]]))


def new_stats():
    return {"calls": 0, "refused": 0, "left_out": 0, "forward": 0.0, "inverse": 0.0, "cycle_spin": 0.0, "spin_bands": 0.0, "group": 0.0, "add": 0.0,
            "norms": 0.0, "group_norm": 0.0, "band_stats": 0.0, "table": 0.0}


def _ratio(stats, key, err, bound, what):
    if bound > 0:
        stats[key] = max(stats[key], err / bound)
    _check(err <= bound, "%s is off by %g, bound %g", what, err, bound)


def _relative(stats, key, got, want, rel, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    for g, w in zip(got, want):
        if np.isnan(w) or np.isinf(w):
            _check((np.isnan(g) and np.isnan(w)) or g == w, "%s = %r, the model's %r", what, g, w)
        else:
            _ratio(stats, key, abs(g - w), rel * abs(w), "%s (%r, the model's %r)" % (what, g, w))


def check_forward(spec, model, subject, stats):
    """the subject's sub-bands against the fp64 composition of the model's image, then the model adopts them"""
    got = subject.raw()
    if spec.prec == "f64":
        ref64, ref32 = model.bands, model.bands
    else:
        ref64, ref32 = model.transform(model.image.astype(np.float64), "full"), model.bands
    for num, (g, r64, r32) in enumerate(zip(got, ref64, ref32)):
        _check(g.dtype == spec.dt and g.shape == r64.shape, "forward: sub-band %d is %s %s", num, g.dtype, g.shape)
        _ratio(stats, "forward", float(np.abs(g.astype(np.float64) - r64).max()), transform_bound(spec, r64, r32), "forward: sub-band %d" % num)
    model.bands = [np.array(g) for g in got]


def check_inverse(spec, model, subject, bands, shift, stats):
    """the subject's image against the fp64 composition of the coefficients `bands` (rolled back by `shift`), then adopted"""
    got = subject.image()
    if spec.prec == "f64":
        ref64 = ref32 = model.image
    else:
        ref64 = model.reconstruct([b.astype(np.float64) for b in bands], "full")
        ref64, ref32 = volume_spin_ref.shift(ref64, [-v for v in shift]), model.image
    _ratio(stats, "inverse", float(np.abs(got.astype(np.float64) - ref64).max()), transform_bound(spec, ref64, ref32), "inverse: the image")
    model.image = np.array(got)


def check_cycle_spin(spec, model, subject, x, op, stats):
    """tests/volume_spin_ref.py, tolerance: K_TOL times the distance between the fp32 and the fp64-accumulated composition, against
    the latter; fp64: 1e-12 max |ref| against the fp64 composition.  The image and the coefficients left behind are adopted."""
    _, variant, mode, value, do_app, normalize, nshifts = op
    kw = dict(mode=mode, beta=value, do_app=do_app, normalize=normalize) if variant == "global" else dict(mode=mode, method="VisuShrink", sigma=value)
    got = subject.image()
    if spec.prec == "f64":
        ref = model.image
        tol = 1e-12 * float(np.abs(ref).max())
    else:
        ref = volume_spin_ref.cycle_spin(x, spec.wname, spec.levels, volume_spin_ref.lattice(nshifts), double=True, **kw)
        tol = volume_spin_ref.K_TOL * float(np.abs(model.image.astype(np.float64) - ref).max())
    _ratio(stats, "cycle_spin", float(np.abs(got.astype(np.float64) - ref).max()), tol, "cycle_spin: the image")
    model.image = np.array(got)
    # The coefficients left behind: the LAST shift's, after its threshold.  Their error is the forward's, carried through the
    # threshold: soft is 1-Lipschitz in the coefficient and in the threshold, hard is the identity or zero away from the
    # threshold.  So the bound is the forward's on the sub-band BEFORE the threshold (what survives a VisuShrink threshold of
    # 60 keeps the rounding error of a coefficient of that size, however small the remainder is) plus the rounding of the
    # threshold itself in pdwt_real (one eps of the largest one; fp64 forms it as the reference does).
    got_bands = subject.raw()
    pre32 = model.transform(volume_spin_ref.shift(x, volume_spin_ref.lattice(nshifts)[-1]))
    if spec.prec == "f64":
        pre64, ref64, slack = pre32, model.bands, 0.0
    else:
        pre64 = model.transform(volume_spin_ref.shift(x.astype(np.float64), volume_spin_ref.lattice(nshifts)[-1]), "full")
        if variant == "global":
            ref64, largest = model._global(pre64, mode, value, do_app, normalize), abs(value)
        else:
            _, table64, ref64 = volume_ops_ref.denoise(pre64, spec.shape, "VisuShrink", mode, value)
            largest = float(np.nanmax(np.abs(table64)))
        slack = float(np.finfo(np.float32).eps) * largest
    for num, (g, r64, p64, p32) in enumerate(zip(got_bands, ref64, pre64, pre32)):
        _check(g.dtype == spec.dt and g.shape == r64.shape, "cycle_spin: sub-band %d is %s %s", num, g.dtype, g.shape)
        _ratio(stats, "spin_bands", float(np.abs(g.astype(np.float64) - r64).max()), transform_bound(spec, p64, p32) + slack,
               "cycle_spin: sub-band %d left behind" % num)
    model.bands = [np.array(g) for g in got_bands]
    if variant == "visu":
        sigma, table = subject.call(("last_thresholds",), None)[1]
        same_bits(sigma, model.sigma, "cycle_spin: the noise level in its slot")
        check_table(spec, model, table, model.table, np.where(np.arange(spec.nbands) > 0, 2 * (2.0 ** -24 if spec.prec == "f32" else U53), np.inf), stats)


def check_table(spec, model, got, want, bound, stats):
    _check(got.dtype == spec.dt and got.shape == (spec.nbands,) and np.isnan(got[0]), "the threshold table is %s %s, entry 0 %r", got.dtype,
           got.shape, got[0] if got.size else None)
    left_out = 0
    for num in range(1, spec.nbands):
        g, r = float(got[num]), float(want[num])
        if np.isinf(bound[num]):
            left_out += 1
        elif np.isnan(r) or np.isinf(r):
            _check((np.isnan(g) and np.isnan(r)) or g == r, "threshold %d = %r, the model's %r", num, g, r)
        else:
            _ratio(stats, "table", abs(g - r), bound[num] * abs(r), "threshold %d (%r, the model's %r)" % (num, g, r))
    stats["left_out"] += left_out
    _check(left_out <= 1, "%d sub-bands of one table are at the max(., eps) edge: the rule allows for one", left_out)
    model.table = np.array(got)


def _close_bands(spec, got, want, kind, stats):
    for num, (g, r) in enumerate(zip(got, want)):
        _check(g.dtype == r.dtype and g.shape == r.shape, "%s: sub-band %d is %s %s", kind, num, g.dtype, g.shape)
        err = np.abs(g.astype(np.longdouble) - r.astype(np.longdouble))
        if kind == "add":  # one ulp of the reference
            ulps = float((err / np.spacing(np.abs(r)).astype(np.longdouble)).max())
            _ratio(stats, "add", ulps, 1.0, "add_wavelet: sub-band %d (ulps)" % num)
        else:
            _ratio(stats, "group", float(err.max()), group_bound(spec, r), "group_soft_threshold: sub-band %d" % num)


def compare_call(spec, subject, model, twin, tmodel, op, stats):
    """One call on both; 1 when it was refused."""
    k = op[0]
    if k == "twin_forward":  # not a generated kind: the named orderings forward the twin after add_wavelet touched its intermediates
        stats["calls"] += 1
        _check(twin.call(("forward",), None)[0] == tmodel.apply(("forward",))[0] == OK, "the twin's forward failed%s", twin.last_error())
        check_forward(spec, tmodel, twin, stats)
        check_all(subject, model, twin, tmodel, "after the twin's forward")
        return 0
    before, image_before, shift_before = model.bands, model.image, model.shift
    got_rc, got = subject.call(op, twin)
    want_rc, want = model.apply(op, tmodel)
    stats["calls"] += 1
    _check(got_rc == want_rc, "returned %r, the model %r%s", got_rc, want_rc, subject.last_error())
    _check(subject.state() == model.state, "state %r, the model's %s", subject.state(), STATE_NAMES[model.state])
    _check(tuple(subject.shift()) == tuple(model.shift), "current_shift %r, the model's %r", tuple(subject.shift()), tuple(model.shift))
    was_refused = refused(op, want_rc)
    if was_refused:
        stats["refused"] += 1
        if k == "get_coeff":
            _check(np.all(got == 7.0), "a refused getter wrote its buffer")
    elif k == "forward":
        check_forward(spec, model, subject, stats)
    elif k == "inverse":
        check_inverse(spec, model, subject, before, shift_before if model.spinning else (0, 0, 0), stats)
    elif k == "cycle_spin":
        check_cycle_spin(spec, model, subject, image_before, op, stats)
    elif k == "group":
        got_bands = subject.raw()
        _close_bands(spec, got_bands, model.bands, "group", stats)
        model.bands = [np.array(g) for g in got_bands]
    elif k == "add_dst":
        got_bands = subject.raw()
        _close_bands(spec, got_bands, model.bands, "add", stats)
        model.bands = [np.array(g) for g in got_bands]
    elif k == "add_src":
        got_bands = twin.raw()
        _close_bands(spec, got_bands, tmodel.bands, "add", stats)
        tmodel.bands = [np.array(g) for g in got_bands]
    elif k in ("norms", "norms_async", "read_norms"):  # tests/test_gpu_volume.py::test_norms: n 2^-53 relative
        n = sum(b.size for b in model.bands)
        _relative(stats, "norms", got, want, n * U53, k)
    elif k == "group_norm":  # tests/test_gpu_volume_prox.py: 2 n 2^-53 relative
        n = sum(b.size for b in model.bands)
        _relative(stats, "group_norm", [got], [want], 2 * n * U53, k)
    elif k in ("band_stats", "read_band_stats"):  # tests/test_gpu_volume_ops.py: 2 n 2^-53 relative, n the sub-band's elements
        _check(np.shape(got) == (spec.nbands, 2), "band_stats has shape %r", np.shape(got))
        for num in range(spec.nbands):
            _relative(stats, "band_stats", got[num], want[num], 2.0 * model.bands[num].size * U53, "%s of sub-band %d" % (k, num))
    elif k in ("estimate_sigma", "read_sigma"):
        same_bits(got, want, k)
    elif k in ("select", "keep", "last_sparsify"):
        same_bits(got[0], want[0], k + ": threshold")
        same_bits(got[1], want[1], k + ": kept")
    elif k == "denoise":
        # in two steps, as tests/test_gpu_volume_ops.py does: sigma exact, the table by its rule, then the sweep bit for bit with
        # the SUBJECT's table
        same_bits(got[0], want[0], "denoise: sigma")
        ref_table, bound = table_bounds(spec, before, want[0], op[1])
        check_table(spec, model, got[1], ref_table, bound, stats)
        model.bands = volume_ops_ref.threshold_bands(before, model.table, op[2])
    elif k == "last_thresholds":
        same_bits(got[0], want[0], k + ": sigma")
        same_bits(got[1], want[1], k + ": table")
    elif k == "current_shift":
        _check(tuple(got) == tuple(want), "current_shift %r, the model's %r", tuple(got), tuple(want))
    elif k == "get_image":
        same_bits(got, want, k)
    elif k == "get_coeff":
        same_bits(got, want, k)
    elif k == "raw_read":
        for num, (g, w) in enumerate(zip(got, want)):
            same_bits(g, w, "raw read of sub-band %d" % num)
    # whatever the call was: nothing else moved
    check_all(subject, model, twin, tmodel, "after the call")
    return 1 if was_refused else 0


def check_all(subject, model, twin, tmodel, when):
    same_bits(subject.image(), model.image, "the image " + when)
    for num, (g, w) in enumerate(zip(subject.raw(), model.bands)):
        same_bits(g, w, "sub-band %d %s" % (num, when))
    for num, (g, w) in enumerate(zip(twin.raw(), tmodel.bands)):
        same_bits(g, w, "the twin's sub-band %d %s" % (num, when))


def run_sequence(spec, ops, make_subject, seed=0, stats=None, model_class=None, at_end=None):
    """Drives a subject -- the library behind the C ABI, the Python class, or another model standing in for it -- and the model
    with `ops`.  make_subject(spec, image, spinning) returns an object with call(op, twin) -> (return value, data), state(),
    shift(), image(), raw(), last_error() and close().  `at_end(subject, twin)` is called before the two are closed.  Returns the
    stats."""
    stats = stats if stats is not None else new_stats()
    image = spec.image(100 + seed)
    subject = twin = None
    try:
        subject = make_subject(spec, image, spec.cycle)
        model = (model_class or VolumeModel)(spec, image)
        _check(subject.state() == model.state == INIT, "a new handle is in state %r", subject.state())
        if spec.cycle:
            model.apply(("spin_on", spec.cycle))
        # the first forward(), and the twin that add_wavelet needs: a second handle of the same image, forwarded (volumes have no clone)
        compare_call(spec, subject, model, _Nothing(), _Nothing(), ("forward",), stats)
        twin = make_subject(spec, image, 0)
        tmodel = (model_class or VolumeModel)(spec, image)
        compare_call(spec, twin, tmodel, _Nothing(), _Nothing(), ("forward",), stats)
        for i, op in enumerate(ops):
            try:
                compare_call(spec, subject, model, twin, tmodel, op, stats)
            except Mismatch as e:
                raise Mismatch("%s, call %d %r: %s\n%s" % (spec.name, i, op, e, as_python(spec, seed, ops, i)))
        # what is left at the end, in whatever state the sequence stopped
        check_all(subject, model, twin, tmodel, "at the end")
        if at_end is not None:
            at_end(subject, twin)
    finally:
        for s in (subject, twin):
            if s is not None:
                s.close()
    return stats


class _Nothing(object):
    """the twin of a handle that has none yet"""
    state = FORWARD
    bands = ()

    def raw(self):
        return ()


class ModelSubject(object):
    """A model behind the subject's interface: tests/test_volume_model_cpu.py runs the comparator with a planted defect standing in
    for the library."""

    def __init__(self, model):
        self.model = model

    def call(self, op, twin):
        rc, data = self.model.apply(op, twin.model if isinstance(twin, ModelSubject) else None)
        if op[0] == "get_coeff" and rc == 0:
            data = np.full(self.model.bands[op[1]].size, 7.0, dtype=self.model.spec.dt)
        return rc, data

    def state(self):
        return self.model.state

    def shift(self):
        return self.model.shift

    def image(self):
        return self.model.image

    def raw(self):
        return self.model.bands

    def last_error(self):
        return ""

    def close(self):
        pass


def model_subject(model_class):
    def make(spec, image, spinning):
        m = model_class(spec, image)
        if spinning:
            m.apply(("spin_on", spinning))
        return ModelSubject(m)
    return make
