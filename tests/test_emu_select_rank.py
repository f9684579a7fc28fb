"""The rank logic of pypwt_amd/csrc/select_kernels.hpp (the K-th largest |c| over several bands: the clamp, the two ends that need
no pass, the accumulated "below" count) on the host against np.sort.

tests/cpu_emu/emu_select_rank.cpp is compiled here with g++ -DPDWT_CPU_EMU -- once for the fp32 keys (three passes), once with
-DPDWT_DOUBLE (six) -- and as a stand-alone program under -fsanitize=address,undefined.  The values are fed as SEVERAL disjoint
ranges of a buffer whose gaps hold huge values (what a band piece must not pick up).  Every comparison is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sparsify_ref
from test_emu_select import vectors

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_select_rank.cpp")
HPP = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc", "select_kernels.hpp")
BASE = ["g++", "-O1", "-g", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-shared"]
_libs = {}


def emu(dtype):
    """libpdwt_emu_select_rank_{f32,f64}.so, rebuilt when the sources are newer."""
    key = np.dtype(dtype).name
    if key in _libs:
        return _libs[key]
    so = os.path.join(HERE, "cpu_emu", "libpdwt_emu_select_rank_%s.so" % ("f64" if dtype == np.float64 else "f32"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HPP)):
        subprocess.check_call(BASE + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", so, SRC])
    lib = C.CDLL(so)
    lib.emu_select_rank.restype = C.c_int
    lib.emu_select_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.POINTER(C.c_ulonglong),
                                    C.POINTER(C.c_ulonglong)]
    _libs[key] = lib
    return lib


def scatter(x, rng):
    """x cut into 1 .. 5 pieces laid out in a larger buffer with gaps of huge values between them: (buffer, starts, lens)."""
    x = np.ascontiguousarray(x)
    npieces = int(min(x.size, rng.integers(1, 6)))
    cuts = np.sort(rng.choice(np.arange(1, x.size), npieces - 1, replace=False)) if npieces > 1 else np.array([], dtype=np.int64)
    pieces = np.split(x, cuts)
    big = np.finfo(x.dtype).max
    buf, starts, lens = [np.full(int(rng.integers(0, 4)), big, dtype=x.dtype)], [], []
    at = buf[0].size
    for p in pieces:
        starts.append(at)
        lens.append(p.size)
        gap = np.full(int(rng.integers(1, 4)), -big, dtype=x.dtype)
        buf += [p, gap]
        at += p.size + gap.size
    return np.concatenate(buf), np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int64)


def run(buf, starts, lens, k):
    thr = np.zeros(1, dtype=buf.dtype)
    kept, key = C.c_ulonglong(), C.c_ulonglong()
    sweeps = emu(buf.dtype.type).emu_select_rank(buf.ctypes.data, starts.ctypes.data, lens.ctypes.data, int(starts.size), int(k),
                                                 thr.ctypes.data, C.byref(kept), C.byref(key))
    return thr[0], int(kept.value), int(key.value), sweeps


def k_values(x, rng):
    """{0, 1, 2, N - 1, N, N + 5} and c - 1, c, c + 1 for every tie boundary c = #(key >= v), v a key of x: all of them for a
    key that occurs more than once and for vectors of at most 64 distinct keys, else 64 drawn at random as well."""
    n = x.size
    allk = sparsify_ref.keys(x).ravel()
    vals, cnt = np.unique(allk, return_counts=True)
    at_least = n - np.concatenate([[0], np.cumsum(cnt)[:-1]])  # elements with key >= vals[j]
    chosen = set(at_least[cnt > 1].tolist())
    chosen |= set(at_least.tolist()) if vals.size <= 64 else set(rng.choice(at_least, 64, replace=False).tolist())
    ks = {0, 1, 2, n - 1, n, n + 5}
    for c in chosen:
        ks |= {c - 1, c, c + 1}
    return sorted(k for k in ks if k >= 0)


def same(a, b):
    return sparsify_ref.same_bits(np.array([a]), np.array([b]))


def check(name, x, rng):
    buf, starts, lens = scatter(x, rng)
    allk = sparsify_ref.keys(x).ravel()
    n = x.size
    seen = set()
    for k in k_values(x, rng):
        thr, kept, key, sweeps = run(buf, starts, lens, k)
        wkey, wthr, wkept = sparsify_ref.select_key(allk, k)
        assert same(thr, wthr), (name, k, thr, wthr)
        assert kept == wkept, (name, k, kept, wkept)
        assert kept >= min(k, n)
        if 0 < k < n:
            assert key == int(wkey) and sweeps == emu(x.dtype.type).emu_select_rank_passes()
        else:
            assert sweeps == 0  # the two ends cost no pass
        seen.add(kept > k)
    return seen


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank_select_equals_sort(dtype):
    lib = emu(dtype)
    assert lib.emu_select_rank_passes() == (3 if dtype == np.float32 else 6)
    rng = np.random.default_rng(17)
    seen = set()
    for name, x in vectors(dtype):
        seen |= check(name, x, rng)
    assert seen == {False, True}  # exact counts and ties that let more than K survive


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank_select_fuzz(dtype):
    rng = np.random.default_rng(23)
    for case in range(300):
        n = int(rng.integers(1, 400))
        kind = case % 4
        if kind == 0:
            x = rng.standard_normal(n)
        elif kind == 1:
            x = rng.integers(-4, 5, n).astype(np.float64)  # many ties and zeros
        elif kind == 2:
            x = rng.standard_normal(n) * np.exp(rng.uniform(-80, 80, n))
        else:
            x = np.round(rng.standard_normal(n), 1)
        x = x.astype(dtype)
        buf, starts, lens = scatter(x, rng)
        allk = sparsify_ref.keys(x).ravel()
        for k in {0, 1, n // 3, n - 1, n, n + 5, int(rng.integers(0, n + 1))}:
            thr, kept, _, _ = run(buf, starts, lens, k)
            _, wthr, wkept = sparsify_ref.select_key(allk, k)
            assert same(thr, wthr) and kept == wkept, (case, k, thr, wthr, kept, wkept)


def test_rank_select_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same vectors through a stand-alone program built with -fsanitize=address,undefined (the runtimes linked statically,
    so that nothing has to be preloaded into a Python process)."""
    for dtype in (np.float32, np.float64):
        exe = str(tmp_path / ("emu_select_rank_san_%s" % np.dtype(dtype).name))
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_SELECT_RANK_MAIN",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
               "-static-libubsan"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", exe, SRC]
        subprocess.check_call(cmd)
        data = str(tmp_path / "vectors.bin")
        rng = np.random.default_rng(29)
        want = []
        with open(data, "wb") as f:
            for name, x in vectors(dtype):
                buf, starts, lens = scatter(x, rng)
                allk = sparsify_ref.keys(x).ravel()
                for k in k_values(x, rng):
                    f.write(np.array([buf.size, starts.size, k], dtype=np.int64).tobytes())
                    f.write(np.stack([starts, lens], axis=1).astype(np.int64).tobytes())
                    f.write(buf.tobytes())
                    want.append((name, k) + sparsify_ref.select_key(allk, k)[1:])
        r = subprocess.run([exe, data], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(want)
        for line, (name, k, wthr, wkept) in zip(lines, want):
            bits, kept = line.split()
            assert int(bits, 16) == int(np.array([wthr]).view(sparsify_ref.key_dtype(dtype))[0]), (name, k, line, wthr)
            assert int(kept) == wkept, (name, k, line, wkept)
