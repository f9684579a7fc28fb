"""The circular shifts of a volume on the host: the geometry, the piece -> (z, r, columns) map, the column wrap and the walk of
pypwt_amd/csrc/volume_shift_kernels.hpp, for vol_circshift_kernel and vol_unshift_acc_kernel alike.

tests/cpu_emu/emu_volume_shift.cpp is compiled here with g++ -DPDWT_CPU_EMU (fp32, and fp64 with -DPDWT_DOUBLE).  It puts source
and destination into heap blocks of exactly the volume's size and walks every workgroup of a launch, wavefront by wavefront and
lane by lane, with the function the kernels walk with.  The outputs are prefilled with NaN: every value must be written exactly
once, be numpy.roll's bit for bit, and every group of four must sit on a 16-byte (fp64: 32-byte) address on both sides.

The same source builds a stand-alone program under -fsanitize=address,undefined; nothing sanitised is loaded into python.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import volume_spin_ref as spin

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_volume_shift.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("volume_shift_kernels.hpp", "kernels_common.hpp")]
BASE = ["g++", "-O1", "-g", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-shared"]
DTYPES = [np.float32, np.float64]
SMALL = [(nz, nr, nc) for nz in (1, 2, 5, 8) for nr in (1, 3, 8) for nc in (1, 2, 3, 4, 7, 8, 12, 13)]
# rows of more than one piece (256 columns), with and without groups; enough pieces for several trips per wavefront
WIDE = [(2, 3, 260), (1, 2, 516), (2, 2, 301), (3, 40, 8), (2, 37, 5)]
RAW = [(-1, -1, -1), (-13, 27, -40), (100, -100, 1000), (7, 8, 9)]  # negative, and beyond the size
_libs = {}


def emu(dtype):
    key = np.dtype(dtype).name
    if key in _libs:
        return _libs[key]
    so = os.path.join(HERE, "cpu_emu", "libpdwt_emu_volume_shift_%s.so" % ("f64" if dtype == np.float64 else "f32"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(BASE + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", so, SRC])
    lib = C.CDLL(so)
    real = C.c_double if dtype == np.float64 else C.c_float
    lib.emu_vs_shift.restype = C.c_longlong
    lib.emu_vs_shift.argtypes = [C.c_int] * 3 + [C.c_longlong] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_vs_acc.restype = C.c_longlong
    lib.emu_vs_acc.argtypes = [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_longlong, real, C.c_void_p, C.c_void_p]
    _libs[key] = lib
    return lib


def axis_shifts(n):
    """Every reduced shift of a small axis, a sample of a longer one (the ends, and both sides of a multiple of four)."""
    return list(range(n)) if n <= 5 else sorted({0, 1, 3, 4, n - 4, n - 1})


def shifts_of(shape):
    return list(itertools.product(*[axis_shifts(n) for n in shape]))


def values(shape, dtype, seed=1):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run_shift(lib, x, s, max_grid=2048, off_in=0, off_out=0):
    out = np.full(x.shape, np.nan, dtype=x.dtype)
    info = np.zeros(7, dtype=np.int64)
    bad = lib.emu_vs_shift(*x.shape, *[int(v) for v in s], max_grid, off_in, off_out, x.ctypes.data, out.ctypes.data, info.ctypes.data)
    return bad, out, info.tolist()


def expected_mode(shape, s, dtype, off_in=0, off_out=0):
    nc, sc = shape[2], s[2] % shape[2]
    wide_out = nc % 4 == 0 and off_out % 4 == 0
    return 2 if wide_out and sc % 4 == 0 and off_in % 4 == 0 else (1 if wide_out else 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_shift_writes_every_value_once_aligned_and_equal_to_numpy_roll(dtype):
    lib = emu(dtype)
    modes = set()
    for shape in SMALL + WIDE:
        x = values(shape, dtype)
        for s in shifts_of(shape) + RAW:
            bad, out, info = run_shift(lib, x, s)
            assert bad == 0, (shape, s, bad)
            assert same_bits(out, spin.shift(x, s)), (shape, s)
            assert info[0] == expected_mode(shape, s, dtype), (shape, s, info)
            assert info[4:] == [v % n for v, n in zip(s, shape)], (shape, s, info)
            assert info[2] == shape[0] * shape[1] * -(-shape[2] // 256) and info[3] == -(-info[2] // 4)
            modes.add(info[0])
    assert modes == {0, 1, 2}


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_capped_grid_strides_over_the_trips_and_a_misaligned_buffer_loses_the_groups(dtype):
    lib = emu(dtype)
    for shape in [(8, 8, 12), (3, 40, 8), (2, 37, 5), (4, 6, 260)]:
        x = values(shape, dtype, 2)
        for s in [(1, 2, 4), (3, 5, 3), (0, 0, 0)]:
            for max_grid in (1, 2):
                bad, out, info = run_shift(lib, x, s, max_grid=max_grid)
                assert bad == 0 and same_bits(out, spin.shift(x, s)), (shape, s, max_grid)
                assert info[1] == min(max_grid, -(-info[3] // 4)) and info[3] > 4 * info[1]  # more than one trip per wavefront
            for off_in, off_out in ((1, 0), (0, 1), (3, 2), (4, 4)):
                bad, out, info = run_shift(lib, x, s, off_in=off_in, off_out=off_out)
                assert bad == 0 and same_bits(out, spin.shift(x, s)), (shape, s, off_in, off_out)
                assert info[0] == expected_mode(shape, s, dtype, off_in, off_out), (shape, s, off_in, off_out, info)


def acc_reference(recs, shifts, w):
    """The kernel's order: w x_0, then acc + w x_s, each product and sum rounded in the volume's precision."""
    acc = None
    for rec, s in zip(recs, shifts):
        term = w * spin.shift(rec, [-v for v in s])
        acc = term if acc is None else acc + term
    return acc


@pytest.mark.parametrize("dtype", DTYPES)
def test_unshift_accumulate_first_and_two_more_equal_the_numpy_sum(dtype):
    lib = emu(dtype)
    w = dtype(1.0) / dtype(3.0)
    modes_seen = set()
    for shape in SMALL + WIDE:
        recs = np.stack([values(shape, dtype, 10 + k) for k in range(3)])
        all_shifts = shifts_of(shape) + RAW
        for i in range(0, len(all_shifts), 3):  # the shifts three by three: every one of them is undone once
            triple = (all_shifts[i:i + 3] + RAW)[:3]
            sh = np.array(triple, dtype=np.int64)
            acc = np.full(shape, np.nan, dtype=dtype)
            modes = np.zeros(3, dtype=np.int64)
            bad = lib.emu_vs_acc(*shape, 3, sh.ctypes.data, 2048, 0, 0, recs.ctypes.data, recs[0].size, w, acc.ctypes.data, modes.ctypes.data)
            assert bad == 0, (shape, triple, bad)
            assert same_bits(acc, acc_reference(recs, triple, w)), (shape, triple)
            # the walk is the shift's with the inverse shift: (N - s) % 4 decides the loads
            assert modes.tolist() == [expected_mode(shape, [-v for v in s], dtype) for s in triple], (shape, triple)
            modes_seen |= set(modes.tolist())
    assert modes_seen == {0, 1, 2}


def test_shifts_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    for dtype in DTYPES:
        exe = str(tmp_path / ("emu_volume_shift_san_%s" % np.dtype(dtype).name))
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_VOLUME_SHIFT_MAIN",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
               "-static-libubsan"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", exe, SRC]
        subprocess.check_call(cmd)
        data, res = str(tmp_path / "records.bin"), str(tmp_path / "out.bin")
        w = dtype(1.0 / 3.0)
        want = []
        with open(data, "wb") as f:
            for shape in SMALL + WIDE:
                x = values(shape, dtype, 3)
                picks = shifts_of(shape)
                for s, max_grid, off_in, off_out in ([(picks[len(picks) // 2], 2048, 0, 0), (picks[-1], 1, 0, 0), (RAW[1], 2048, 0, 0),
                                                      (picks[len(picks) // 3], 2048, 1, 3)]):
                    f.write(np.array(list(shape) + list(s) + [max_grid, off_in, off_out], dtype=np.int64).tobytes())
                    f.write(x.tobytes())
                    three = [s, (s[0] + 1, s[1] + 2, s[2] + 3), (-5 - s[0], -s[1], 7 - s[2])]
                    want.append((shape, s, spin.shift(x, s), acc_reference([x, x, x], three, w)))
        r = subprocess.run([exe, data, res], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(want)
        got = np.fromfile(res, dtype=dtype)
        at = 0
        for line, (shape, s, shifted, acc) in zip(lines, want):
            assert line.split() == ["0", "0"], (shape, s, line)
            n = shifted.size
            assert same_bits(got[at:at + n].reshape(shape), shifted), (shape, s)
            assert same_bits(got[at + n:at + 2 * n].reshape(shape), acc), (shape, s)
            at += 2 * n
        assert at == got.size
