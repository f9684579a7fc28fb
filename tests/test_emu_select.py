"""The pass logic of pypwt_amd/csrc/select_kernels.hpp (digits, bucket walk, the two middle ranks) on the host against np.sort.

tests/cpu_emu/emu_select.cpp is compiled here with g++ -DPDWT_CPU_EMU -- once for the fp32 keys (three passes), once with
-DPDWT_DOUBLE (six) -- and as a stand-alone program under -fsanitize=address,undefined.  Every comparison is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_select.cpp")
HPP = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc", "select_kernels.hpp")
BASE = ["g++", "-O1", "-g", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-shared"]
_libs = {}


def emu(dtype):
    """libpdwt_emu_select_{f32,f64}.so, rebuilt when the sources are newer."""
    key = np.dtype(dtype).name
    if key in _libs:
        return _libs[key]
    so = os.path.join(HERE, "cpu_emu", "libpdwt_emu_select_%s.so" % ("f64" if dtype == np.float64 else "f32"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HPP)):
        subprocess.check_call(BASE + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", so, SRC])
    lib = C.CDLL(so)
    lib.emu_select_median.restype = C.c_int
    lib.emu_select_median.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    _libs[key] = lib
    return lib


def run(x, skip_zeros=True):
    x = np.ascontiguousarray(x)
    med, sig = C.c_double(), C.c_double()
    mode = emu(x.dtype.type).emu_select_median(x.ctypes.data, x.size, int(skip_zeros), C.byref(med), C.byref(sig))
    return med.value, sig.value, mode


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def vectors(dtype):
    """(name, values) of every case the select can get wrong."""
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    rng = np.random.default_rng(11)
    out = []
    for n in (1, 2, 3, 4, 63, 64, 65, 4096, 4097):
        out.append(("normal%d" % n, (rng.standard_normal(n) * 10).astype(dt)))
    out.append(("all_equal", np.full(1000, dt(-3.25))))
    out.append(("all_equal_odd", np.full(999, dt(7.5))))
    out.append(("all_zero", np.zeros(300, dtype=dt)))
    out.append(("signed_zeros", np.array([0.0, -0.0] * 50, dtype=dt)))
    half = (rng.standard_normal(2000)).astype(dt)
    half[::2] = 0.0
    half[1::4] *= 1.0
    half[::6] = -0.0
    out.append(("half_zeros", half))
    # the two middle elements one ulp apart and in DIFFERENT first-pass buckets: they straddle a power of two
    two = dt(2.0)
    below = np.nextafter(two, dt(0))
    v = np.concatenate([np.linspace(0.1, 1.5, 499).astype(dt), [below, two], np.linspace(2.5, 9.0, 499).astype(dt)])
    out.append(("straddle_pow2", rng.permutation(v).astype(dt)))
    # ... and parting in the SECOND and in the LAST pass only
    a = dt(1.0) + dt(2.0) ** -5
    v = np.concatenate([np.full(10, dt(0.5)), [np.nextafter(a, dt(0)), a], np.full(10, dt(3.0))]).astype(dt)
    out.append(("straddle_late", -v))
    v = np.concatenate([np.full(7, dt(1.0)), [dt(1.5), np.nextafter(dt(1.5), dt(2))], np.full(7, dt(8.0))]).astype(dt)
    out.append(("one_ulp_last_pass", v))
    # ties around the middle
    out.append(("ties", np.array([1, 2, 2, 2, 2, 3, 3, 9], dtype=dt)))
    out.append(("ties2", np.array([5, 1, 1, 5, 5, 1], dtype=dt)))
    # denormals, inf, a NaN
    den = np.array([fi.smallest_subnormal, -fi.smallest_subnormal * 3, np.nextafter(fi.tiny, dt(0)), fi.tiny, -fi.tiny * 2, 0.0], dtype=dt)
    out.append(("denormals", den))
    out.append(("denormals_even", den[:4]))
    out.append(("inf_nan", np.array([1.0, -np.inf, np.nan, 2.0, np.inf, -3.0], dtype=dt)))
    out.append(("mostly_inf", np.array([np.inf, -np.inf, np.inf, 1.0], dtype=dt)))
    out.append(("nan_middle", np.array([np.nan, np.nan, np.nan, 1.0], dtype=dt)))
    out.append(("max", np.array([fi.max, -fi.max, 1.0, fi.max], dtype=dt)))
    out.append(("edge_vector", adaptive_ref.ops_ref.edge_vector(2.5, dt)))
    out.append(("wide_range", (rng.standard_normal(5000) * np.exp(rng.uniform(-60, 60, 5000))).astype(dt)))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_select_equals_sort(dtype):
    lib = emu(dtype)
    assert lib.emu_select_passes() == (3 if dtype == np.float32 else 6)
    seen_modes = set()
    for name, x in vectors(dtype):
        for skip in (True, False):
            med, sig, mode = run(x, skip)
            want = adaptive_ref.median_abs(x, skip)
            assert same(med, want), (name, skip, med, want)
            assert same(sig, want / adaptive_ref.SIGMA_DENOMINATOR), (name, skip)
            seen_modes.add(mode)
    assert seen_modes == {0, 1, 2}  # shared bucket to the end, parted on the way, odd count
    assert run(np.zeros(300, dtype=dtype), True)[:2] == (0.0, 0.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_select_fuzz(dtype):
    rng = np.random.default_rng(3)
    for k in range(300):
        n = int(rng.integers(1, 400))
        kind = k % 4
        if kind == 0:
            x = rng.standard_normal(n)
        elif kind == 1:
            x = rng.integers(-4, 5, n).astype(np.float64)  # many ties and zeros
        elif kind == 2:
            x = rng.standard_normal(n) * np.exp(rng.uniform(-80, 80, n))
        else:
            x = np.round(rng.standard_normal(n), 1)
        x = x.astype(dtype)
        for skip in (True, False):
            assert same(run(x, skip)[0], adaptive_ref.median_abs(x, skip)), (k, skip)


def test_select_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same vectors through a stand-alone program built with -fsanitize=address,undefined (the runtimes linked statically,
    so that nothing has to be preloaded into a Python process)."""
    for dtype in (np.float32, np.float64):
        exe = str(tmp_path / ("emu_select_san_%s" % np.dtype(dtype).name))
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_SELECT_MAIN",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
               "-static-libubsan"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", exe, SRC]
        subprocess.check_call(cmd)
        data = str(tmp_path / "vectors.bin")
        want = []
        with open(data, "wb") as f:
            for name, x in vectors(dtype):
                for skip in (1, 0):
                    x = np.ascontiguousarray(x)
                    f.write(np.array([x.size, skip], dtype=np.int64).tobytes())
                    f.write(x.tobytes())
                    want.append((name, skip, adaptive_ref.median_abs(x, bool(skip))))
        r = subprocess.run([exe, data], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        got = [float.fromhex(l) for l in r.stdout.split()]
        assert len(got) == len(want)
        for g, (name, skip, w) in zip(got, want):
            assert same(g, w), (name, skip, g, w)
