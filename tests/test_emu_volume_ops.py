"""The index math of pypwt_amd/csrc/volume_ops_kernels.hpp on the host: the range table of a volume's K-term operators, the
piece -> range map of its workgroups, and the (level, band, slice) -> sub-band map of its table expansion.

tests/cpu_emu/emu_volume_ops.cpp is compiled here with g++ -DPDWT_CPU_EMU (fp32, and fp64 with -DPDWT_DOUBLE).  It lays the
per-level arenas out as the level plans do, fills every sub-band with its `num` and everything else -- the intermediates, the
padding -- with a huge sentinel, and walks every workgroup of the table the way sweep_range does: each swept element must be
visited exactly once, no sentinel at all, and every group of four on a 16-byte (fp64: 32-byte) address.  The emulated select
and keep sweep over the ranges equal tests/sparsify_ref.py exactly, at the tie-boundary K's of tests/test_emu_select_rank.py.

The same source builds a stand-alone program under -fsanitize=address,undefined whose arenas are heap blocks of exactly the
coefficient regions' size; nothing sanitised is loaded into python.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sparsify_ref
import volume_ops_ref
import volume_ref
from test_emu_select_rank import k_values

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_volume_ops.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("volume_ops_kernels.hpp", "select_kernels.hpp", "kernels_common.hpp")]
BASE = ["g++", "-O1", "-g", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-shared"]
# (shape, levels)
SHAPES = [((2, 2, 2), 1), ((5, 64, 64), 2), ((9, 10, 13), 1), ((3, 3, 3), 1), ((64, 48, 40), 3), ((7, 5, 6), 2)]
DTYPES = [np.float32, np.float64]
_libs = {}


def emu(dtype):
    key = np.dtype(dtype).name
    if key in _libs:
        return _libs[key]
    so = os.path.join(HERE, "cpu_emu", "libpdwt_emu_volume_ops_%s.so" % ("f64" if dtype == np.float64 else "f32"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(BASE + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", so, SRC])
    lib = C.CDLL(so)
    lib.emu_vol_num_of.argtypes = [C.c_int] * 5
    lib.emu_vol_locate.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3
    lib.emu_vol_locate.restype = None
    lib.emu_vol_walk.restype = C.c_longlong
    lib.emu_vol_walk.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    lib.emu_vol_keep_largest.argtypes = [C.c_int] * 5 + [C.c_longlong, C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
    _libs[key] = lib
    return lib


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_swept_element_once_and_no_sentinel(dtype):
    lib = emu(dtype)
    for shape, L in SHAPES:
        sizes = [int(np.prod(s)) for s in volume_ref.band_shapes(shape, L)]
        for do_app in (0, 1):
            for which, min_chunk in ((0, 8192), (1, 4096)):
                counts = np.full(1 + 7 * L, -1, dtype=np.int64)
                info = np.zeros(4, dtype=np.int64)
                bad = lib.emu_vol_walk(*shape, L, do_app, which, counts.ctypes.data, info.ctypes.data)
                assert bad == 0, (shape, L, do_app, which, bad)
                want = list(sizes)
                if not do_app:
                    want[0] = 0
                assert counts.tolist() == want, (shape, L, do_app, which)
                nranges, chunk, blocks, total = info.tolist()
                assert nranges == 4 * L + 1 and chunk >= min_chunk and chunk % 1024 == 0 and total == sum(sizes)
                assert blocks >= nranges - (0 if do_app else 1)  # at least one workgroup per range


def test_sub_band_map_is_the_numbering_of_the_volume():
    lib = emu(np.float32)
    for L in (1, 2, 3, 5):
        for level in range(1, L + 1):
            for half in (1, 2, 3, 17):
                seen = {}
                for band in range(4):
                    for img in range(2 * half):
                        num = lib.emu_vol_num_of(level, L, band, img, half)
                        keys = [k for k, (h, b) in volume_ref.SUB.items() if h == (img >= half) and b == band]
                        assert len(keys) == 1
                        if keys[0] == "aaa":
                            assert num == (0 if level == L else -1), (level, L, band, img)
                        else:
                            assert num == volume_ref.num_of(level, keys[0]), (level, L, band, img)
                        seen.setdefault(num, 0)
                        seen[num] += 1
                assert all(c == half for c in seen.values()) and len(seen) == 8
        for num in range(1 + 7 * L):  # and back
            lv, hf, bd = C.c_int(), C.c_int(), C.c_int()
            lib.emu_vol_locate(num, L, C.byref(lv), C.byref(hf), C.byref(bd))
            assert lib.emu_vol_num_of(lv.value, L, bd.value, hf.value * 3, 3) == num


def values(dtype, n, kind, rng):
    if kind == 0:
        x = rng.standard_normal(n) * 50.0
    elif kind == 1:
        x = rng.integers(-4, 5, n).astype(np.float64)  # many ties and zeros
        x[::9] = -0.0
    else:
        x = rng.standard_normal(n) * np.exp(rng.uniform(-60, 60, n))
        x[rng.integers(0, n)] = np.nan
        x[rng.integers(0, n)] = np.inf
        x[rng.integers(0, n)] = -np.inf
    return x.astype(dtype)


def split(flat, shape, L):
    out, at = [], 0
    for s in volume_ref.band_shapes(shape, L):
        n = int(np.prod(s))
        out.append(flat[at:at + n].reshape(s))
        at += n
    return out


def run(lib, shape, L, do_app, k, flat):
    work = flat.copy()
    thr = np.zeros(1, dtype=flat.dtype)
    kept = C.c_ulonglong()
    sweeps = lib.emu_vol_keep_largest(*shape, L, do_app, int(k), work.ctypes.data, thr.ctypes.data, C.byref(kept))
    return sweeps, thr, int(kept.value), work


@pytest.mark.parametrize("dtype", DTYPES)
def test_select_and_keep_over_the_ranges_equal_the_reference(dtype):
    lib = emu(dtype)
    rng = np.random.default_rng(31)
    passes = 3 if dtype == np.float32 else 6
    more = set()
    for shape, L in SHAPES:
        total = sum(int(np.prod(s)) for s in volume_ref.band_shapes(shape, L))
        for kind in range(3):
            flat = values(dtype, total, kind, rng)
            bands = split(flat, shape, L)
            for do_app in (0, 1):
                swept = np.concatenate([b.ravel() for b in bands[0 if do_app else 1:]])
                ks = k_values(swept, rng)
                if len(ks) > 40:  # the six fixed ones, and a sample of the tie boundaries
                    ks = sorted(set(ks[:3] + ks[-3:] + rng.choice(ks, 34, replace=False).tolist()))
                for k in ks:
                    sweeps, thr, kept, work = run(lib, shape, L, do_app, k, flat)
                    wthr, wkept, want = volume_ops_ref.keep_largest(bands, k, do_app)
                    assert sweeps == (passes if 0 < k < swept.size else 0), (shape, kind, do_app, k, sweeps)
                    assert sparsify_ref.same_bits(thr, wthr) and kept == int(wkept[0]), (shape, kind, do_app, k, thr, wthr, kept, wkept)
                    for num, (g, w) in enumerate(zip(split(work, shape, L), want)):
                        assert sparsify_ref.same_bits(g, w), (shape, kind, do_app, k, num)
                    more.add(kept > k)
    assert more == {False, True}


def test_volume_ops_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    for dtype in DTYPES:
        exe = str(tmp_path / ("emu_volume_ops_san_%s" % np.dtype(dtype).name))
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_VOLUME_OPS_MAIN",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
               "-static-libubsan"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", exe, SRC]
        subprocess.check_call(cmd)
        data, res = str(tmp_path / "records.bin"), str(tmp_path / "out.bin")
        rng = np.random.default_rng(37)
        want = []
        with open(data, "wb") as f:
            for shape, L in SHAPES:
                total = sum(int(np.prod(s)) for s in volume_ref.band_shapes(shape, L))
                for kind in range(3):
                    flat = values(dtype, total, kind, rng)
                    bands = split(flat, shape, L)
                    for do_app in (0, 1):
                        n = volume_ops_ref.count(bands, do_app)
                        for k in (0, 1, n // 3, n - 1, n, n + 5):
                            f.write(np.array(list(shape) + [L, do_app, k, total], dtype=np.int64).tobytes())
                            f.write(flat.tobytes())
                            wthr, wkept, out = volume_ops_ref.keep_largest(bands, k, do_app)
                            want.append((shape, kind, do_app, k, wthr, int(wkept[0]), np.concatenate([b.ravel() for b in out])))
        r = subprocess.run([exe, data, res], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(want)
        got = np.fromfile(res, dtype=dtype)
        at = 0
        for line, (shape, kind, do_app, k, wthr, wkept, out) in zip(lines, want):
            bad_hist, bad_keep, status, bits, kept = line.split()
            assert int(bad_hist) == 0 and int(bad_keep) == 0 and int(status) >= 0, (shape, kind, do_app, k, line)
            assert int(bits, 16) == int(wthr.view(sparsify_ref.key_dtype(dtype))[0]) and int(kept) == wkept, (shape, kind, do_app, k, line)
            assert sparsify_ref.same_bits(got[at:at + out.size], out), (shape, kind, do_app, k)
            at += out.size
        assert at == got.size
