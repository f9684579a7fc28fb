"""The depth-axis kernels of a volume (pypwt_amd/csrc/dwt3_axis_kernels.hpp) on the host against the CPU oracle.

tests/cpu_emu/emu_axis.cpp is compiled here with g++ -DPDWT_CPU_EMU (fp32, and fp64 with -DPDWT_DOUBLE): the kernels' tile
functions -- periodised source slice, segment bounds, the synthesis' tap-to-output map, odd depths -- run workgroup by workgroup
over the launcher's grid.  The reference is the depth step of tests/volume_ref.py: the oracle's one-level 1D transform along
the depth axis, in fp64.  Depths below the filter length (the periodic index wraps more than once) are part of the sweep.

Every even length from 2 to 40 taps is instantiated (the launchers' own list, PDWT_EVEN_HLENS) and swept: 2 taps with haar (the
oracle restates the reference's hard-coded Haar butterfly there, a custom 2-tap bank has no oracle), 4 to 40 taps with the banks of
tests/tap_banks.py, in which no tap is below 0.079 -- a dropped or shifted tap is thousands of times outside the bound.  The six
built-in wavelets stay beside them: they pin the real tables, db20's tiny taps included, to the same path.

Bound: every output is a dot product of at most hlen products, so |error| <= hlen * eps * sum|taps| * max|input| (the
standard bound of a recursive sum, gamma_n ~ n eps), for the data's eps; a wrong index is off by the size of the data.

The same source builds a stand-alone program under -fsanitize=address,undefined whose buffers are heap blocks of exactly
the input's and output's size; nothing sanitised is loaded into python.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
import tap_banks

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_axis.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("dwt3_axis_kernels.hpp", "axis_common.hpp", "kernels_common.hpp", "strip_walk.hpp")]
BASE = ["g++", "-O2", "-g", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU"]
WNAME = {2: "haar", 4: "db2", 8: "db4", 16: "db8", 18: "db9", 40: "db20"}
LENGTHS = tuple(range(2, 41, 2))  # every instantiation
# a case is a built-in wavelet's name or the length of a tap_banks bank; "haar" stands for 2 taps in both lists
CASES = sorted(WNAME.values(), key=lambda w: oracle.filters(w)[0]) + [n for n in LENGTHS if n > 2]
PLANES = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4099)
SLOTS = (1, 16, 2048)  # resident workgroups the chooser is asked for: one long walk ... as many segments as it will cut
_libs = {}


def emu(dtype):
    key = np.dtype(dtype).name
    if key in _libs:
        return _libs[key]
    so = os.path.join(HERE, "cpu_emu", "libpdwt_emu_axis_%s.so" % ("f64" if dtype == np.float64 else "f32"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(BASE + ["-shared"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", so, SRC])
    lib = C.CDLL(so)
    lib.emu_axis_width.argtypes = [C.c_longlong, C.c_int]
    lib.emu_axis_steps.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.emu_axis_seg.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.emu_axis_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    _libs[key] = lib
    return lib


def div2(n):
    return (n + (n & 1)) // 2


def variants(lib, Nz, P, hlen, inverse):
    """(seg, width) of every launch shape: both access widths, every segment length the chooser returns, and 1 and 2 forced."""
    out = []
    for width in sorted({1, lib.emu_axis_width(P, hlen)}):
        segs = {1, 2} | {lib.emu_axis_seg(Nz, P, hlen, width, inverse, s) for s in SLOTS}
        steps = lib.emu_axis_steps(Nz, hlen, inverse)
        assert all(1 <= s <= max(steps, 1) for s in segs - {2}), (segs, steps)
        out += [(s, width) for s in sorted(segs)]
    return out


def run(lib, x, out_slices, Nz, P, hlen, lo, hi, seg, width, inverse):
    out = np.full((out_slices, P), np.nan, dtype=x.dtype)
    rc = lib.emu_axis_run(x.ctypes.data, out.ctypes.data, Nz, P, hlen, lo.ctypes.data, hi.ctypes.data, seg, width, int(inverse))
    assert rc == 0, (Nz, P, hlen, seg, width, inverse)
    return out


def filters_of(case, dtype):
    """(hlen, dec_lo, dec_hi, rec_lo, rec_hi) in the data's type: a built-in wavelet by name, or the bank of that many taps."""
    if isinstance(case, str):
        return oracle.filters(case, dtype)
    filt = tap_banks.bank(case, 900 + case)
    return (filt[0],) + tuple(t.astype(dtype) for t in filt[1:])


def reference(x64, Nz, P, filt, inverse):
    """The oracle's one-level 1D transform along the depth axis in fp64 with the bank `filt` (its taps as the kernel got them);
    x64: [Nz][P] forward, [2 div2(Nz)][P] inverse.  2 taps: by name -- the oracle's Haar butterfly."""
    w, f64 = ("haar", None) if filt[0] == 2 else (None, (filt[0],) + tuple(t.astype(np.float64) for t in filt[1:]))
    if not inverse:
        lo, hi = oracle.forward(np.ascontiguousarray(x64.T), w, 1, ndim=1, double="full", filt=f64)
        return np.concatenate([np.asarray(lo).reshape(P, -1).T, np.asarray(hi).reshape(P, -1).T])
    h = div2(Nz)
    halves = [np.ascontiguousarray(x64[:h].T), np.ascontiguousarray(x64[h:].T)]
    return np.asarray(oracle.inverse(halves, (P, Nz), w, 1, ndim=1, double="full", filt=f64)).reshape(P, Nz).T


def test_every_even_length_is_built_and_no_other():
    """emu_axis_run instantiates the launchers' list: 2 .. 40 even; an odd or longer length is refused (non-zero)."""
    lib = emu(np.float32)
    x = np.zeros((2, 4), dtype=np.float32)
    taps = np.zeros(64, dtype=np.float32)
    for hlen in range(0, 45):
        out = np.zeros((2, 4), dtype=np.float32)
        rc = lib.emu_axis_run(x.ctypes.data, out.ctypes.data, 2, 4, hlen, taps.ctypes.data, taps.ctypes.data, 1, 1, 0)
        assert (rc == 0) == (hlen in LENGTHS), hlen
    assert sorted({oracle.filters(c)[0] if isinstance(c, str) else c for c in CASES}) == list(LENGTHS)


# (ids: a built-in wavelet keeps its length, as before the banks came; "bank<n>" is the n-tap bank)
@pytest.mark.parametrize("case", CASES, ids=[str(oracle.filters(c)[0]) if isinstance(c, str) else "bank%d" % c for c in CASES])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_depth_kernels_equal_the_oracle_along_depth(dtype, case):
    lib = emu(dtype)
    eps = float(np.finfo(dtype).eps)
    filt = filters_of(case, dtype)
    hlen, dlo, dhi, rlo, rhi = filt
    if not isinstance(case, str):
        assert min(float(np.abs(t).min()) for t in filt[1:]) >= 0.079  # every tap counts
    rng = np.random.default_rng(100 + hlen)
    shapes = 0
    for inverse in (False, True):
        lo, hi = (rlo, rhi) if inverse else (dlo, dhi)
        taps = max(float(np.abs(lo).sum()), float(np.abs(hi).sum()))
        for P in PLANES:
            for Nz in range(1, 42):
                n_in = 2 * div2(Nz) if inverse else Nz
                n_out = Nz if inverse else 2 * div2(Nz)
                x = (rng.standard_normal((n_in, P)) * 100).astype(dtype)
                want = reference(x.astype(np.float64), Nz, P, filt, inverse)
                assert want.shape == (n_out, P)
                tol = 2 * hlen * eps * taps * float(np.abs(x).max())  # (2: both half-bands meet in one synthesis output)
                for seg, width in variants(lib, Nz, P, hlen, inverse):
                    got = run(lib, x, n_out, Nz, P, hlen, lo, hi, seg, width, inverse)
                    err = np.abs(got.astype(np.float64) - want).max()  # NaN: an output the walk never wrote
                    assert err <= tol, (Nz, P, hlen, seg, width, inverse, err, tol)
                    shapes += 1
    assert shapes >= 2 * len(PLANES) * 41 * 3


def test_segment_chooser_covers_the_walk():
    """ceil(steps / seg) segments of seg steps cover every step, for every size of the sweep and from one slot to many."""
    lib = emu(np.float32)
    for hlen in LENGTHS:
        for inverse in (0, 1):
            for Nz in range(1, 42):
                steps = lib.emu_axis_steps(Nz, hlen, inverse)
                assert steps == (div2(Nz) if not inverse else (Nz - 1 + (0 if (hlen // 2) & 1 else 1)) // 2 + 1)
                for P in PLANES:
                    for slots in SLOTS + (0, 7, 100000):
                        seg = lib.emu_axis_seg(Nz, P, hlen, 1, inverse, slots)
                        assert 1 <= seg <= steps
    # a big plane and few slices: one segment; tiny planes and many slices: the depth axis is cut
    assert lib.emu_axis_seg(8, 4096 * 4096, 8, 4, 0, 2048) == 4
    assert lib.emu_axis_seg(4096, 64, 8, 4, 0, 2048) < 64


def test_depth_kernels_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Heap blocks of exactly the input's and output's size: every residue of P mod 4, both parities of the depth, depths below
    the filter length, both widths, segments of 1, 2 and the chooser's.  The outputs equal the unsanitised build's, bit for bit."""
    for dtype in (np.float32, np.float64):
        lib = emu(dtype)
        exe = str(tmp_path / ("emu_axis_san_%s" % np.dtype(dtype).name))
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_AXIS_MAIN",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
               "-static-libubsan"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", exe, SRC]
        subprocess.check_call(cmd)
        rng = np.random.default_rng(7)
        data, res = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
        want = []
        with open(data, "wb") as f:
            for hlen in LENGTHS:
                _, dlo, dhi, rlo, rhi = filters_of("haar" if hlen == 2 else hlen, dtype)
                for inverse in (0, 1):
                    lo, hi = (rlo, rhi) if inverse else (dlo, dhi)
                    for P in (1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 258):
                        for Nz in (1, 2, 3, 8, 9, 41):
                            n_in = 2 * div2(Nz) if inverse else Nz
                            n_out = Nz if inverse else 2 * div2(Nz)
                            x = rng.standard_normal((n_in, P)).astype(dtype)
                            for seg, width in variants(lib, Nz, P, hlen, inverse):
                                f.write(np.array([Nz, P, hlen, seg, width, inverse], dtype=np.int64).tobytes())
                                f.write(np.ascontiguousarray(lo).tobytes() + np.ascontiguousarray(hi).tobytes() + x.tobytes())
                                want.append(run(lib, x, n_out, Nz, P, hlen, lo, hi, seg, width, inverse))
        r = subprocess.run([exe, data, res], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        assert int(r.stdout.split()[-1]) == len(want)
        got = np.fromfile(res, dtype=dtype)
        flat = np.concatenate([w.ravel() for w in want])
        assert got.shape == flat.shape and not np.isnan(flat).any()
        assert np.array_equal(got, flat)
