"""`Wavelets3D`: the separable 3D DWT of a volume on the GPU, decimated or -- ``do_swt=1`` -- stationary (the pdwt_volume_* block
of include/pypwt_amd.h).

The reference stops at two dimensions ("3D is not handled at the moment", pdwt/README.md:29); this class follows the 2D
`Wavelets` in everything that carries over -- level clamping, state rules, thresholds, norms -- with the boundary rule of the
rest of the library (pywt's "periodization").  ctypes binding only.

    W = Wavelets3D(vol, "db2", 3); W.forward(); W.soft_threshold(10); W.inverse(); W.coeffs; W.image
    W.forward(); W.denoise("BayesShrink"); W.inverse()        # the threshold of every sub-band from the data, on the device
    W.forward(); W.keep_largest(fraction=0.05); W.inverse()   # best K-term approximation
    W = Wavelets3D(vol, "db4", 3, do_swt=1); W.forward(); W.soft_threshold(10); W.inverse()   # translation-invariant denoising
    W.group_soft_threshold(t); W.proj_linf(t); W.shrink(t); W.add_wavelet(W_old, -0.5); W.group_norm()   # the proximal steps
    W = Wavelets3D(vol, "db4", 3); W.cycle_spin(n=8, beta=10); W.image   # cycle spinning: the mean of the denoiser over 8 shifts
"""
import itertools
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, handle_t
from .wavelets import DeviceArray, _device_array, _ptr

KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")  # pywt.wavedecn's keys with axes (z, y, x), sorted: the order of `num`


def volume_layout(shape, wname, levels, lib=None):
    """(levels after clamping, [(depth, rows, cols) of every coefficient index]) of a volume of `shape`: a pure host
    computation (pdwt_volume_layout), no device needed."""
    lib = lib or _lib.load()
    nz, nr, nc = (int(n) for n in shape)
    nlev = C.c_int(0)
    cap = 1 + 7 * max(int(levels), 1)
    dims = (C.c_int * (3 * cap))()
    n = check(lib.pdwt_volume_layout(nz, nr, nc, wname.encode("ascii"), int(levels), C.byref(nlev), dims, cap), "volume_layout", lib)
    return nlev.value, [tuple(dims[3 * k:3 * k + 3]) for k in range(n)]


def volume_layout_swt(shape, wname, levels, dtype=np.float32, lib=None):
    """(levels after clamping, bytes of device memory) of a STATIONARY volume of `shape` and `dtype`: a pure host computation
    (pdwt_volume_layout_swt), no device needed -- (3 + 8 L) volumes, so worth asking before the volume is created."""
    lib = lib or _lib.load()
    nz, nr, nc = (int(n) for n in shape)
    nlev, nbytes = C.c_int(0), C.c_longlong(0)
    check(lib.pdwt_volume_layout_swt(nz, nr, nc, wname.encode("ascii"), int(levels), C.byref(nlev), C.byref(nbytes),
                                     np.dtype(dtype).itemsize), "volume_layout_swt", lib)
    return nlev.value, nbytes.value


def spin_footprint(shape, dtype=np.float32, lib=None):
    """Bytes of device memory the first `Wavelets3D.cycle_spin` of a volume of `shape` and `dtype` allocates (the kept source and
    the running mean: two volumes, each padded to 256 bytes): a pure host computation (pdwt_volume_spin_footprint)."""
    lib = lib or _lib.load()
    nz, nr, nc = (int(n) for n in shape)
    out = C.c_size_t(0)
    check(lib.pdwt_volume_spin_footprint(nz, nr, nc, np.dtype(dtype).itemsize, C.byref(out)), "spin_footprint", lib)
    return int(out.value)


def spin_lattice(n):
    """The first `n` (at most 64) shifts (sz, sr, sc) of the fixed lattice of `Wavelets3D.cycle_spin`: the eight points of
    {0, 1}^3 in lexicographic order -- (0,0,0), (0,0,1), (0,1,0), ..., (1,1,1) --, then the points of {0, 1, 2, 3}^3 in
    lexicographic order without those eight.  An (n, 3) int32 array."""
    n = int(n)
    if not 1 <= n <= 64:
        raise ValueError("spin_lattice: n must be 1 .. 64, got %d" % n)
    first = list(itertools.product((0, 1), repeat=3))
    rest = [p for p in itertools.product(range(4), repeat=3) if max(p) > 1]
    return np.array((first + rest)[:n], dtype=np.int32)


class Wavelets3D(object):
    """3D DWT plan of one volume [Nz][Nr][Nc].

    vol : C-contiguous 3D numpy array of the instance's dtype (float32), or a device array / torch tensor on the GPU
          (``__cuda_array_interface__``), copied device-to-device
    wname, levels : as for `Wavelets`; the levels are clamped by the reference's rule on the smallest of the three sizes
    device : device ordinal, -1 = the current one;  stream : a HIP stream handle to run on, None = a private stream
    do_swt : 1 = the stationary (undecimated, a-trous) transform: pywt.swtn / pywt.iswtn with axes (z, y, x).  Every band then has
          the volume's shape, any size from 2 on each axis is taken (odd ones too), and the device holds (3 + 8 levels) volumes
          (`volume_layout_swt` tells beforehand).  ``coeffs`` keeps its shape ``[A_L, d_1, ..., d_L]``; pywt.swtn's list is,
          coarsest level first, a dict per level that also holds 'aaa': ``[dict(d_L, aaa=A_L)] + [dict(d_l, aaa=...) for l = L-1 .. 1]``
          where the 'aaa' of a level below L is an intermediate this class does not keep -- pywt.iswtn reads only the first
          dict's.  The operators that choose a threshold or a sparsity from the data (`band_stats`, `estimate_sigma`,
          `threshold_bands`, `denoise`, `select_magnitude`, `keep_largest`, `norms_device`) are not built for it and raise
          NotImplementedError.

    Cycle spinning -- a fresh random circular shift per ``forward()``, undone by ``inverse()``, as `Wavelets(do_cycle_spinning=1)`
    does in 2D -- is turned on with ``set_cycle_spinning(1, seed)``; ``cycle_spin`` is the averaged denoiser.

    Coefficient index ``num``: 0 = the approximation A_L, then 1 + 7 (l - 1) + k with level 1 the FINEST and k over the keys
    'aad', 'ada', 'add', 'daa', 'dad', 'dda', 'ddd' -- pywt.wavedecn's, axes (z, y, x).  ``coeffs`` is ``[A, d_1, ..., d_L]``
    with every d_l a dict over those keys; pywt.wavedecn's order is ``[c[0]] + c[:0:-1]``.
    """
    _variant = "f32"
    _dtype = np.float32

    def __init__(self, vol, wname, levels, device=-1, stream=None, do_swt=0):
        self._h = None
        self.do_swt = 1 if do_swt else 0
        self.do_cycle_spinning = 0
        self._lib = _lib.load(self._variant)
        dev = _device_array(vol, self._dtype)
        if dev is not None:
            shape = dev[1]
        else:
            vol = np.asarray(vol)
            shape = vol.shape
        if len(shape) != 3:
            raise ValueError("Wavelets3D: the volume must have three dimensions, got shape %s" % (shape,))
        if dev is None:
            vol = self._checkarray(vol, shape)
        self.shape = tuple(int(n) for n in shape)
        self.wname = wname
        h = handle_t()
        if dev is not None:
            self._order_producer(dev, device)
        src = C.c_void_p(dev[0]) if dev is not None else _ptr(vol)
        create = self._lib.pdwt_volume_create_swt if self.do_swt else self._lib.pdwt_volume_create
        check(create(src, self.shape[0], self.shape[1], self.shape[2], wname.encode("ascii"), int(levels),
                     0 if dev is not None else 1, int(device), C.c_void_p(stream) if stream else None, C.byref(h)), "Wavelets3D", self._lib)
        self._h = h
        self.levels = self.info()["nlevels"]
        self.hlen = self.info()["hlen"]
        if self.do_swt:
            self._shapes = [self.shape] * (1 + 7 * self.levels)
        else:
            self._shapes = volume_layout(self.shape, wname, self.levels, self._lib)[1]

    # ---- helpers
    def _check(self, rc, what=""):
        return check(rc, what, self._lib)

    @classmethod
    def _checkarray(cls, arr, shp):
        if arr.dtype != cls._dtype or not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("Wavelets3D: the array must be C-contiguous %s" % np.dtype(cls._dtype).name)
        if tuple(arr.shape) != tuple(shp):
            raise ValueError("The array does not have the correct shape (expected %s, got %s)" % (str(tuple(shp)), str(arr.shape)))
        return arr

    def _order_producer(self, dev, device=None):
        """A device source is copied on the volume's own stream: order the copy after the source's producer."""
        if not dev[2]:
            return
        if dev[2][0] == "stream":
            self._check(self._lib.pdwt_sync_producer(-1, C.c_void_p(dev[2][1]), 0))
        else:
            owner = int(self._lib.pdwt_device_of_pointer(C.c_void_p(dev[0])))
            self._check(self._lib.pdwt_sync_producer(owner if owner >= 0 else -1, None, 1))

    def _source(self, arr, shp):
        dev = _device_array(arr, self._dtype)
        if dev is not None:
            if tuple(dev[1]) != tuple(int(n) for n in shp):  # the exact shape, as for host arrays: nothing is reinterpreted
                raise ValueError("The array does not have the correct shape (expected %s, got %s)" % (str(tuple(shp)), str(dev[1])))
            self._order_producer(dev)
            return C.c_void_p(dev[0]), 1
        arr = self._checkarray(np.asarray(arr), shp)
        return _ptr(arr), 0  # (the upload has finished when the call returns: nothing to keep alive)

    # ---- introspection
    def info(self):
        v = [C.c_int() for _ in range(6)]
        self._check(self._lib.pdwt_volume_get_info(self._h, *[C.byref(x) for x in v]))
        out = dict(zip(("Nz", "Nr", "Nc", "nlevels", "hlen", "state"), (x.value for x in v)))
        out["do_swt"] = self.do_swt  # (the constructor's argument: no further call)
        return out

    def __repr__(self):
        return "<%s %s %s levels=%d%s>" % (type(self).__name__, "x".join(str(n) for n in self.shape), self.wname, self.levels,
                                           " swt" if self.do_swt else "")

    def _not_for_swt(self, method):
        if self.do_swt:
            raise NotImplementedError("Wavelets3D.%s is not built for stationary volumes (do_swt=1)" % method)

    def depth_schedule(self, level):
        """(columns per thread, steps per depth segment forward, inverse) of the depth passes of `level` (1 .. levels).  Stationary
        volumes: the columns of the analysis, and the steps per segment of an orbit walk."""
        v = [C.c_int() for _ in range(3)]
        self._check(self._lib.pdwt_volume_depth_schedule(self._h, int(level), *[C.byref(x) for x in v]), "depth_schedule")
        return tuple(x.value for x in v)

    def _set_filters(self, filt):
        """Test plumbing (pdwt_volume_set_filters): `filt` = (hlen, dec_lo, dec_hi, rec_lo, rec_hi) replaces the bank of the depth
        passes and of every level's 2D plan; hlen must be the volume's own.  Custom banks on volumes are not part of the product."""
        taps = [np.ascontiguousarray(t, dtype=self._dtype) for t in filt[1:5]]
        if any(t.shape != (int(filt[0]),) for t in taps):
            raise ValueError("Wavelets3D._set_filters: four filters of %d taps expected" % int(filt[0]))
        rp = C.POINTER(self._lib.pdwt_real)
        self._check(self._lib.pdwt_volume_set_filters(self._h, int(filt[0]), *[C.cast(t.ctypes.data, rp) for t in taps]), "_set_filters")

    def _set_depth_segments(self, level, seg_fwd, seg_inv):
        """Test plumbing (pdwt_volume_set_depth_segments): steps per depth segment of `level`, forward and inverse; 0 restores the
        chooser's value."""
        self._check(self._lib.pdwt_volume_set_depth_segments(self._h, int(level), int(seg_fwd), int(seg_inv)), "_set_depth_segments")

    def _depth_width(self, level, inverse):
        """Test plumbing (pdwt_volume_depth_width): columns per thread of the depth analysis (inverse false) or synthesis of `level`."""
        return self._check(self._lib.pdwt_volume_depth_width(self._h, int(level), 1 if inverse else 0), "_depth_width")

    def band_shape(self, num):
        return self._shapes[num]

    @property
    def nbands(self):
        return len(self._shapes)

    # ---- transforms
    def forward(self, vol=None):
        """Forward transform of ``vol`` if given, else of the current image."""
        if vol is not None:
            self.set_image(vol)
        self._check(self._lib.pdwt_volume_forward(self._h), "forward")

    def inverse(self):
        """Coefficients -> ``image``.  As for `Wavelets`, a second call in a row does nothing but warn, and the coefficients
        cannot be read or thresholded afterwards until forward() (or set_coeff of the approximation)."""
        rc = self._lib.pdwt_volume_inverse(self._h)
        if rc == _lib.ERR_STATE:
            print("Warning: " + _lib.last_error(self._lib))
            return
        self._check(rc, "inverse")

    # ---- circular shifts and cycle spinning
    def circshift(self, sz, sr, sc):
        """image <- numpy.roll(image, (sz, sr, sc), axis=(0, 1, 2)), on the device and in place as the caller sees it
        (``image_device`` stays where it is).  Shifts may be negative or beyond the size.  The image must be current: after
        ``forward()`` it raises; run ``inverse()`` or ``set_image`` first."""
        self._check(self._lib.pdwt_volume_circshift(self._h, int(sz), int(sr), int(sc)), "circshift")

    def set_cycle_spinning(self, on=1, seed=None):
        """``on``: every ``forward()`` first shifts the image circularly by a fresh pseudo-random (sz, sr, sc) and the matching
        ``inverse()`` shifts the result back -- one random shift per iteration of an iterative reconstruction, what
        `Wavelets(..., do_cycle_spinning=1)` does in 2D.  ``seed`` (None = 0) decides the draws: the same seed gives the same
        shifts.  ``last_shift`` tells the shift.  Decimated volumes only (a stationary one raises NotImplementedError).  Off by
        default.  Returns self."""
        self._check(self._lib.pdwt_volume_set_cycle_spinning(self._h, 1 if on else 0, int(seed or 0) & (2 ** 64 - 1)), "set_cycle_spinning")
        self.do_cycle_spinning = 1 if on else 0
        return self

    @property
    def last_shift(self):
        """(sz, sr, sc): what ``forward()`` shifted the image by (``set_cycle_spinning``; the sum of the draws when several
        forwards ran in a row); (0, 0, 0) once ``inverse()`` has shifted back, after ``set_image`` and without cycle spinning."""
        v = (C.c_int * 3)()
        self._check(self._lib.pdwt_volume_current_shift(self._h, v), "last_shift")
        return tuple(int(x) for x in v)

    def cycle_spin(self, shifts=None, n=8, mode="soft", beta=None, method=None, sigma=None, do_threshold_appcoeffs=0, normalize=0,
                   skip_zeros=True):
        """Cycle spinning (Coifman and Donoho): image <- the mean over K circular shifts s of  unshift_s(inverse(theta(forward(
        shift_s(image))))) -- the decimated denoiser made (nearly) translation invariant at K times its cost and two extra volumes
        of memory (`spin_footprint`), all on the device.

        shifts : (K, 3) integers (sz, sr, sc); None = the first ``n`` points of `spin_lattice` (n = 8: all shifts by 0 or 1)
        mode : "soft" or "hard"
        beta : the global threshold, as ``soft_threshold(beta, do_threshold_appcoeffs, normalize)`` / ``hard_threshold``;
        method : instead of ``beta``, "BayesShrink" or "VisuShrink" as ``denoise(method, sigma, mode, skip_zeros)``: with
                 ``sigma=None`` every shift estimates its own noise level.  Exactly one of ``beta`` and ``method``.
        The image must be current (not after ``forward()``); afterwards the state is that after ``inverse()``.  Returns self; the
        result is ``image``."""
        if (beta is None) == (method is None):
            raise ValueError("cycle_spin: expected exactly one of beta (a global threshold) and method (\"BayesShrink\" / \"VisuShrink\")")
        op = self._choice(self._THRESHOLD_MODES, mode, "mode")
        m = -1 if method is None else self._choice(self._DENOISE_METHODS, method, "method")
        sh = spin_lattice(n) if shifts is None else np.ascontiguousarray(np.asarray(shifts))
        if sh.dtype.kind not in "iu" or sh.ndim != 2 or sh.shape[1] != 3:
            raise ValueError("cycle_spin: shifts must be a (K, 3) integer array, got %s %s" % (sh.dtype, sh.shape))
        sh = np.ascontiguousarray(sh, dtype=np.int32)
        arg = None
        if sigma is not None:
            sg = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma, dtype=np.float64)))
            if sg.shape != (1,):
                raise ValueError("cycle_spin: sigma must be one number (a volume is one image)")
            arg = sg.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self._lib.pdwt_volume_cycle_spin_async(self._h, sh.shape[0], sh.ctypes.data_as(C.POINTER(C.c_int)), op,
                                                           float(beta) if beta is not None else 0.0, int(do_threshold_appcoeffs),
                                                           int(normalize), m, arg, 1 if skip_zeros else 0), "cycle_spin")
        return self

    # ---- data
    @property
    def image(self):
        res = np.zeros(self.shape, dtype=self._dtype)
        n = self._lib.pdwt_volume_get_image(self._h, _ptr(res))
        if n != res.size:
            raise RuntimeError("Wavelets3D.image: expected %d values, got %d (%s)" % (res.size, n, _lib.last_error(self._lib)))
        return res

    def set_image(self, vol):
        """Replace the image (the coefficients are not updated; run forward())."""
        src, on_device = self._source(vol, self.shape)
        self._check(self._lib.pdwt_volume_set_image(self._h, src, on_device), "set_image")

    def coeff_only(self, num):
        """One sub-band as a numpy array [depth][rows][cols]."""
        if num < 0 or num >= self.nbands:
            raise ValueError("Wavelets3D.coeff_only: coefficient index %d out of range (0 .. %d)" % (num, self.nbands - 1))
        res = np.zeros(self._shapes[num], dtype=self._dtype)
        n = self._lib.pdwt_volume_get_coeff(self._h, _ptr(res), int(num))
        if n != res.size:
            raise RuntimeError("Wavelets3D.coeff_only: expected %d values, got %d (%s)" % (res.size, n, _lib.last_error(self._lib)))
        return res

    @property
    def coeffs(self):
        """``[A, d_1, ..., d_L]``: d_l is a dict keyed 'aad' ... 'ddd', level 1 the finest (pywt.wavedecn: ``[c[0]] + c[:0:-1]``)."""
        out = [self.coeff_only(0)]
        for l in range(1, self.levels + 1):
            out.append({k: self.coeff_only(1 + 7 * (l - 1) + i) for i, k in enumerate(KEYS)})
        return out

    def set_coeff(self, arr, num):
        """Overwrite one sub-band from a host array or a device array of its shape."""
        if num < 0 or num >= self.nbands:
            raise ValueError("Wavelets3D.set_coeff: coefficient index %d out of range (0 .. %d)" % (num, self.nbands - 1))
        src, on_device = self._source(arr, self._shapes[num])
        self._check(self._lib.pdwt_volume_set_coeff(self._h, src, int(num), on_device), "set_coeff")

    # ---- operators
    def _threshold(self, fn, beta, do_threshold_appcoeffs, normalize):
        rc = fn(self._h, float(beta), int(do_threshold_appcoeffs), int(normalize))
        if rc == _lib.ERR_STATE:
            print("Warning: Wavelets3D(): " + _lib.last_error(self._lib))
            return
        self._check(rc)

    def soft_threshold(self, beta, do_threshold_appcoeffs=0, normalize=0):
        """sign(x) (|x| - t)_+ on the details (and on the approximation with ``do_threshold_appcoeffs``); ``normalize``: t is
        divided by sqrt(2) at each scale."""
        self._threshold(self._lib.pdwt_volume_soft_threshold, beta, do_threshold_appcoeffs, normalize)

    def hard_threshold(self, beta, do_threshold_appcoeffs=0, normalize=0):
        """x 1_{|x| > t}"""
        self._threshold(self._lib.pdwt_volume_hard_threshold, beta, do_threshold_appcoeffs, normalize)

    def group_soft_threshold(self, beta, do_threshold_appcoeffs=0, normalize=0):
        """Group soft threshold: at every level and position the seven detail coefficients 'aad' .. 'ddd' (and A_L at the last
        level with ``do_threshold_appcoeffs``) shrink together by max(1 - t / ||g||_2, 0); ``normalize`` as for ``soft_threshold``.
        One launch over all levels, decimated and stationary volumes alike."""
        self._threshold(self._lib.pdwt_volume_group_soft_threshold, beta, do_threshold_appcoeffs, normalize)

    def proj_linf(self, beta, do_threshold_appcoeffs=1):
        """Projection on the l-infinity ball of radius beta: sign(x) min(|x|, beta) on the details, and on A_L with the flag."""
        self._refused(self._lib.pdwt_volume_proj_linf(self._h, float(beta), int(do_threshold_appcoeffs)))

    def shrink(self, beta, do_threshold_appcoeffs=1):
        """x / (1 + beta) on the details, and on A_L with the flag: the proximal map of beta/2 ||.||_2^2."""
        self._refused(self._lib.pdwt_volume_shrink(self._h, float(beta), int(do_threshold_appcoeffs)))

    def add_wavelet(self, W, alpha=1.0):
        """c += alpha * c_W on every sub-band.  ``W`` must be a volume of the same class, shape, wavelet, levels, transform kind
        and device (else it raises, with nothing done); the work runs on this volume's stream, after what is queued on ``W``'s."""
        if not isinstance(W, Wavelets3D) or W._variant != self._variant:
            raise ValueError("Wavelets3D.add_wavelet: the right operand must be a %s" % type(self).__name__)
        self._refused(self._lib.pdwt_volume_add_wavelet(self._h, W._h, float(alpha)))

    def group_norm(self, do_threshold_appcoeffs=0):
        """The l2,1 norm ``group_soft_threshold`` is the proximal map of: the sum over levels and positions of the Euclidean norm of
        the group, accumulated in float64 in a fixed order (two calls give the same bits).  Blocks."""
        out = C.c_double(0.0)
        self._check(self._lib.pdwt_volume_group_norm(self._h, int(do_threshold_appcoeffs), C.byref(out)), "group_norm")
        return float(out.value)

    def group_norm_device(self, out=None, do_threshold_appcoeffs=0):
        """``group_norm`` as one float64 ON THE DEVICE, enqueued and not waited for: ``out`` if given (a device array of one
        float64), else a (1,) view of the volume's own slot."""
        arg, view = self._out(out, 1, "group_norm_device")
        slot = C.c_void_p()
        self._check(self._lib.pdwt_volume_group_norm_async(self._h, int(do_threshold_appcoeffs), arg, C.byref(slot)), "group_norm_device")
        return view if view is not None else self._view(slot.value, (1,), np.float64)

    def norms(self):
        """(sum |c|, sum c^2) over all coefficients, accumulated in float64."""
        out = (C.c_double * 2)()
        self._check(self._lib.pdwt_volume_norms(self._h, out), "norms")
        return float(out[0]), float(out[1])

    def norm1(self):
        return self.norms()[0]

    def norm2sq(self):
        return self.norms()[1]

    # ---- operators that choose the threshold, or the sparsity, from the data: `Wavelets`' methods with the volume as ONE image
    _DENOISE_METHODS = {"bayesshrink": 0, "visushrink": 1}
    _THRESHOLD_MODES = {"soft": 0, "hard": 1}

    @staticmethod
    def _choice(table, name, what):
        try:
            return table[str(name).lower()]
        except KeyError:
            raise ValueError("unknown %s %r (expected one of %s)" % (what, name, ", ".join(sorted(table))))

    def _refused(self, rc):
        """As for `soft_threshold` after inverse(): a warning, nothing done."""
        if rc == _lib.ERR_STATE:
            print("Warning: Wavelets3D(): " + _lib.last_error(self._lib))
            return True
        self._check(rc)
        return False

    def _adaptive_slots(self):
        st, sg, tb = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._lib.pdwt_volume_adaptive_slots(self._h, C.byref(st), C.byref(sg), C.byref(tb)), "pdwt_volume_adaptive_slots")
        return st.value, sg.value, tb.value

    def _sparsify_slots(self):
        th, kp = C.c_void_p(), C.c_void_p()
        self._check(self._lib.pdwt_volume_sparsify_slots(self._h, C.byref(th), C.byref(kp)), "pdwt_volume_sparsify_slots")
        return th.value, kp.value

    def _view(self, ptr, shape, dtype):
        return DeviceArray(self, ptr, shape, dtype, self._stream())

    def _out(self, out, count, which):
        """(argument for the C call, view to return) of an optional caller-owned float64 device array."""
        if out is None:
            return C.c_void_p(None), None
        dev = _device_array(out, np.float64)
        if dev is None or int(np.prod(dev[1])) < count:
            raise ValueError("%s: `out` must be a device array of %d float64" % (which, count))
        return C.c_void_p(dev[0]), out

    def _read(self, addr, shape, dtype):
        """Device memory copied to the host on the volume's stream (waits for it)."""
        host = np.zeros(shape, dtype=dtype)
        self._check(self._lib.pdwt_volume_read(self._h, host.ctypes.data_as(C.c_void_p), C.c_void_p(int(addr)), host.nbytes), "pdwt_volume_read")
        return host

    @staticmethod
    def _addr(view):
        return int(view.__cuda_array_interface__["data"][0])

    def band_stats(self, out=None):
        """(sum |c|, sum c^2) of every sub-band as float64 ON THE DEVICE: a (nbands, 2) device array -- ``out`` if given, else a
        view of the volume's own slot.  Slices and levels are pooled on the device; two calls give the same bits."""
        self._not_for_swt("band_stats")
        arg, view = self._out(out, 2 * self.nbands, "band_stats")
        self._check(self._lib.pdwt_volume_band_stats_async(self._h, arg), "band_stats")
        return view if view is not None else self._view(self._adaptive_slots()[0], (self.nbands, 2), np.float64)

    def read_band_stats(self, view=None):
        """What ``band_stats`` left on the device, copied to the host (waits for the volume's stream): (nbands, 2) float64."""
        self._not_for_swt("read_band_stats")
        return self._read(self._adaptive_slots()[0] if view is None else self._addr(view), (self.nbands, 2), np.float64)

    def estimate_sigma(self, skip_zeros=True, out=None):
        """The noise level sigma = median(|ddd_1|) / 0.6745 over the WHOLE finest 'ddd' sub-band (``num`` 7; the rule of
        skimage.restoration.denoise_wavelet for n-D data), as float64 ON THE DEVICE: a (1,) device array.  The median is exact;
        ``skip_zeros`` (default, as skimage does) leaves exact zeros out of it."""
        self._not_for_swt("estimate_sigma")
        arg, view = self._out(out, 1, "estimate_sigma")
        self._check(self._lib.pdwt_volume_estimate_sigma_async(self._h, 1 if skip_zeros else 0, arg), "estimate_sigma")
        return view if view is not None else self._view(self._adaptive_slots()[1], (1,), np.float64)

    def read_sigma(self, view=None):
        """What ``estimate_sigma`` (or ``denoise``) left on the device, copied to the host: (1,) float64."""
        self._not_for_swt("read_sigma")
        return self._read(self._adaptive_slots()[1] if view is None else self._addr(view), (1,), np.float64)

    def threshold_bands(self, betas, mode="soft"):
        """Soft or hard threshold with a threshold of its own per sub-band: ``betas`` is a (nbands,) array of the instance's dtype
        -- a numpy array or any device-array holder ``set_coeff`` accepts.  A NaN entry leaves that sub-band untouched (entry 0 is
        the approximation A_L)."""
        self._not_for_swt("threshold_bands")
        op = self._choice(self._THRESHOLD_MODES, mode, "mode")
        dev = _device_array(betas, self._dtype)
        if dev is not None:
            if int(np.prod(dev[1])) != self.nbands:
                raise ValueError("threshold_bands: expected %d thresholds, got %d" % (self.nbands, int(np.prod(dev[1]))))
            self._order_producer(dev)
            self._refused(self._lib.pdwt_volume_threshold_bands(self._h, op, C.c_void_p(dev[0]), 1))
            return
        t = np.ascontiguousarray(np.asarray(betas, dtype=self._dtype))
        if t.shape != (self.nbands,):
            raise ValueError("threshold_bands: expected thresholds of shape (%d,), got %s" % (self.nbands, str(t.shape)))
        self._refused(self._lib.pdwt_volume_threshold_bands(self._h, op, _ptr(t), 0))

    def denoise(self, method="BayesShrink", sigma=None, mode="soft", skip_zeros=True):
        """Adaptive wavelet shrinkage of the current coefficients (run ``forward`` before and ``inverse`` after it).
        ``method``: "BayesShrink" (a threshold per detail sub-band) or "VisuShrink" (sigma sqrt(2 ln(Nz Nr Nc))); ``sigma``: the
        noise level, None = ``estimate_sigma``; ``mode``: "soft" or "hard".  Nothing goes through the host; ``last_thresholds``
        shows what was applied."""
        self._not_for_swt("denoise")
        m = self._choice(self._DENOISE_METHODS, method, "method")
        op = self._choice(self._THRESHOLD_MODES, mode, "mode")
        arg = None
        if sigma is not None:
            sg = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma, dtype=np.float64)))
            if sg.shape != (1,):
                raise ValueError("denoise: sigma must be one number (a volume is one image)")
            arg = sg.ctypes.data_as(C.POINTER(C.c_double))
        self._refused(self._lib.pdwt_volume_denoise_async(self._h, m, op, arg, 1 if skip_zeros else 0))

    def last_thresholds(self):
        """(sigma, thresholds) of the last ``denoise``, copied to the host (waits for the volume's stream): sigma is (1,) float64,
        thresholds (nbands,) of the instance's dtype with NaN at index 0 (the approximation is left alone)."""
        self._not_for_swt("last_thresholds")
        _, sg, tb = self._adaptive_slots()
        return self._read(sg, (1,), np.float64), self._read(tb, (self.nbands,), self._dtype)

    def _sparsify_count(self, do_threshold_appcoeffs):
        """N: the elements of the swept sub-bands (the 7 L detail sub-bands, and A_L when asked for), from the band shapes."""
        return sum(int(np.prod(shp)) for shp in self._shapes[0 if do_threshold_appcoeffs else 1:])

    def _sparsify_k(self, what, k, fraction, do_threshold_appcoeffs):
        expected = "%s: expected exactly one of k (an int >= 0) and fraction (a number in [0, 1])" % what
        if (k is None) == (fraction is None):
            raise ValueError(expected)
        if fraction is not None:
            try:
                f = float(fraction)
            except (TypeError, ValueError):
                raise ValueError(expected + ", got fraction=%r" % (fraction,))
            if not 0.0 <= f <= 1.0:  # a NaN fails both comparisons
                raise ValueError(expected + ", got fraction=%r" % (fraction,))
            return int(round(f * self._sparsify_count(do_threshold_appcoeffs)))
        try:
            arr = np.asarray(k)
            if arr.dtype.kind not in "iu" or arr.size != 1 or int(arr.reshape(-1)[0]) < 0 or int(arr.reshape(-1)[0]) > np.iinfo(np.int64).max:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(expected + ", got k=%r" % (k,))
        return int(arr.reshape(-1)[0])

    def select_magnitude(self, k=None, fraction=None, do_threshold_appcoeffs=0):
        """The K-th largest ``|c|`` over the detail sub-bands of all levels (and A_L with ``do_threshold_appcoeffs``), EXACT, and
        how many elements are at least that large: ``(threshold, kept)`` as device views of the volume's slots, (1,) of the
        instance's dtype and (1,) uint64.  ``fraction``: K = round(fraction * N).  Read-only; ``last_sparsify`` copies the pair to
        the host.  K = 0 gives (+inf, 0), K >= N gives (0, N)."""
        self._not_for_swt("select_magnitude")
        kk = self._sparsify_k("select_magnitude", k, fraction, do_threshold_appcoeffs)
        self._check(self._lib.pdwt_volume_select_magnitude_async(self._h, kk, 1 if do_threshold_appcoeffs else 0, None, None), "select_magnitude")
        th, kp = self._sparsify_slots()
        return self._view(th, (1,), self._dtype), self._view(kp, (1,), np.uint64)

    def keep_largest(self, k=None, fraction=None, do_threshold_appcoeffs=0):
        """Best K-term approximation of the volume: keep, bit for bit, the K coefficients of largest magnitude (ties with the K-th
        all survive; NaNs count as larger than +inf) and set the rest to +0.0 -- the select above and one sweep over all levels,
        nothing through the host.  After ``inverse()`` it warns and does nothing, like every threshold."""
        self._not_for_swt("keep_largest")
        kk = self._sparsify_k("keep_largest", k, fraction, do_threshold_appcoeffs)
        self._refused(self._lib.pdwt_volume_keep_largest_async(self._h, kk, 1 if do_threshold_appcoeffs else 0))

    def last_sparsify(self):
        """(threshold, kept) of the last ``select_magnitude`` / ``keep_largest``, copied to the host (waits for the volume's
        stream): (1,) of the instance's dtype and (1,) uint64."""
        self._not_for_swt("last_sparsify")
        th, kp = self._sparsify_slots()
        return self._read(th, (1,), self._dtype), self._read(kp, (1,), np.uint64)

    def norms_device(self, out=None):
        """(sum |c|, sum c^2) over all coefficients as two float64 ON THE DEVICE, enqueued and not waited for (``norms`` blocks):
        the fixed-order sum of the ``band_stats`` rows.  Returns ``out`` if given, else a view of the volume's own slot."""
        self._not_for_swt("norms_device")
        arg, view = self._out(out, 2, "norms_device")
        self._check(self._lib.pdwt_volume_norms_async(self._h, arg), "norms_device")
        if view is not None:
            return view
        return self._view(self._adaptive_slots()[0] + 2 * self.nbands * 8, (2,), np.float64)

    def read_norms(self, view=None):
        """The two float64 a ``norms_device`` call left on the device, copied to the host (waits for the volume's stream)."""
        self._not_for_swt("read_norms")
        addr = self._adaptive_slots()[0] + 2 * self.nbands * 8 if view is None else self._addr(view)
        res = self._read(addr, (2,), np.float64)
        return float(res[0]), float(res[1])

    # ---- device views
    def _stream(self):
        return self._lib.pdwt_volume_stream(self._h) or 0

    @property
    def image_device(self):
        """Zero-copy `DeviceArray` view of the image."""
        return DeviceArray(self, self._lib.pdwt_volume_image_ptr(self._h), self.shape, self._dtype, self._stream())

    def coeff_device(self, num):
        """Zero-copy `DeviceArray` view of one sub-band [depth][rows][cols]."""
        ptr = self._lib.pdwt_volume_coeff_ptr(self._h, int(num))
        if not ptr:
            raise ValueError("Wavelets3D.coeff_device: coefficient index %d out of range" % num)
        return DeviceArray(self, ptr, self._shapes[num], self._dtype, self._stream())

    def synchronize(self):
        self._check(self._lib.pdwt_volume_synchronize(self._h))

    def cleanup(self):
        if getattr(self, "_h", None):
            self._lib.pdwt_volume_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass


class Wavelets3D64(Wavelets3D):
    """The same on libpypwt_amd_f64.so: float64 volumes and coefficients."""
    _variant = "f64"
    _dtype = np.float64
