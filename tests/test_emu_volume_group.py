"""The group operators of a volume on the host: the table, the piece -> (level, positions) map, the head / groups / tail split and
the arithmetic of pypwt_amd/csrc/volume_ops_kernels.hpp (vol_group_*), for both layouts.

tests/cpu_emu/emu_volume_group.cpp is compiled here with g++ -DPDWT_CPU_EMU (fp32, and fp64 with -DPDWT_DOUBLE).  It lays the
coefficients out as a decimated and as a stationary volume do, fills every sub-band with its `num` and everything else -- the
intermediates, the gaps, the padding -- with a huge sentinel, and walks every workgroup of the table with the function the kernels
walk with: every member of every group exactly once, no sentinel read or written, every group of four on a 16-byte (fp64:
32-byte) address for EVERY member.  The emulated threshold and norm equal tests/volume_prox_ref.py within the bounds of the GPU
test (tests/test_gpu_volume_prox.py).

The same source builds a stand-alone program under -fsanitize=address,undefined whose arenas are heap blocks of exactly the
coefficient regions' size; nothing sanitised is loaded into python.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ops_ref
import volume_prox_ref as prox
import volume_ref
import volume_swt_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_volume_group.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("volume_ops_kernels.hpp", "select_kernels.hpp", "kernels_common.hpp")]
BASE = ["g++", "-O1", "-g", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-shared"]
# (shape, levels, stationary): n_l = 3, 1, 2, 0 (mod 4) and a tiny one; several pieces with a ragged last one; stationary
SHAPES = [((9, 10, 13), 1, 0), ((6, 6, 10), 1, 0), ((6, 6, 4), 1, 0), ((16, 16, 16), 2, 0), ((7, 5, 6), 2, 0), ((40, 48, 44), 2, 0),
          ((5, 7, 9), 2, 1), ((9, 10, 13), 1, 1), ((3, 3, 5), 1, 1), ((8, 8, 8), 3, 1), ((24, 24, 28), 3, 1)]
DTYPES = [np.float32, np.float64]
_libs = {}


def emu(dtype):
    key = np.dtype(dtype).name
    if key in _libs:
        return _libs[key]
    so = os.path.join(HERE, "cpu_emu", "libpdwt_emu_volume_group_%s.so" % ("f64" if dtype == np.float64 else "f32"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(BASE + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", so, SRC])
    lib = C.CDLL(so)
    for name in ("emu_vg_walk", "emu_vg_soft", "emu_vg_norm"):
        getattr(lib, name).restype = C.c_longlong
    lib.emu_vg_walk.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    lib.emu_vg_soft.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    lib.emu_vg_norm.argtypes = [C.c_int] * 6 + [C.c_void_p, C.POINTER(C.c_double)]
    _libs[key] = lib
    return lib


def shapes_of(shape, L, swt):
    return volume_swt_ref.band_shapes(shape, L) if swt else volume_ref.band_shapes(shape, L)


def split(flat, shape, L, swt):
    out, at = [], 0
    for s in shapes_of(shape, L, swt):
        n = int(np.prod(s))
        out.append(flat[at:at + n].reshape(s))
        at += n
    return out


def values(dtype, shape, L, swt, rng):
    """Coefficients whose groups straddle the threshold, with a few groups of all zeros."""
    total = sum(int(np.prod(s)) for s in shapes_of(shape, L, swt))
    x = (rng.standard_normal(total) * 10.0).astype(dtype)
    bands = split(x, shape, L, swt)
    for l in range(1, L + 1):
        for k in range(7):
            bands[1 + 7 * (l - 1) + k].reshape(-1)[::11] = 0  # (views of x: position 0, 11, ... of every member: zero groups)
    return x


def bound(ref_band, dtype):
    """The GPU test's bound of one sub-band."""
    eps = 5e-6 if dtype == np.float32 else 8 * 2.0 ** -52
    return eps * max(float(np.abs(ref_band).max()), 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_member_of_every_group_once_aligned_and_no_sentinel(dtype):
    lib = emu(dtype)
    paths = set()
    for shape, L, swt in SHAPES:
        sizes = [int(np.prod(s)) for s in shapes_of(shape, L, swt)]
        for do_app in (0, 1):
            counts = np.full(1 + 7 * L, -1, dtype=np.int64)
            info = np.zeros(5, dtype=np.int64)
            bad = lib.emu_vg_walk(*shape, L, swt, do_app, counts.ctypes.data, info.ctypes.data)
            assert bad == 0, (shape, L, swt, do_app, bad)
            want = list(sizes)
            if not do_app:
                want[0] = 0
            assert counts.tolist() == want, (shape, L, swt, do_app)
            levels, chunk, blocks, total, singles = info.tolist()
            n_l = [sizes[1 + 7 * (l - 1)] for l in range(1, L + 1)]
            assert levels == L and chunk >= 2048 and chunk % 1024 == 0 and total == sum(n_l)
            assert blocks == sum(-(-n // chunk) for n in n_l)
            assert singles == sum(n for n in n_l if n % 4)
            paths |= {"groups" if n % 4 == 0 else "singles" for n in n_l}
            paths |= {"several pieces"} if any(n > chunk and n % chunk for n in n_l) else set()
    assert paths == {"groups", "singles", "several pieces"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_emulated_threshold_and_norm_equal_the_reference(dtype):
    lib = emu(dtype)
    rng = np.random.default_rng(41)
    for shape, L, swt in SHAPES:
        flat = values(dtype, shape, L, swt, rng)
        bands = split(flat, shape, L, swt)
        n = flat.size
        for do_app in (0, 1):
            for normalize in (0, 1):
                beta = 26.0  # the norm of seven N(0, 10) values is about 26: half of the groups go
                betas = np.array(ops_ref.level_betas(beta, L, normalize, np.dtype(dtype).type), dtype=dtype)
                work = flat.copy()
                assert lib.emu_vg_soft(*shape, L, swt, do_app, betas.ctypes.data, work.ctypes.data) == 0, (shape, swt, do_app)
                want = prox.group_soft(bands, L, beta, do_app, normalize)
                for num, (g, w) in enumerate(zip(split(work, shape, L, swt), want)):
                    err = float(np.abs(g.astype(np.longdouble) - w.astype(np.longdouble)).max())
                    assert err <= bound(w, dtype), (shape, swt, do_app, normalize, num, err)
                if not do_app:
                    assert np.array_equal(work[:bands[0].size], flat[:bands[0].size])  # A_L is no member: untouched
                zero = next(b for b in split(work, shape, L, swt)[1:])
                assert zero.reshape(-1)[0] == 0  # a group of zeros stays zero (no 0 / 0)
            out = C.c_double()
            assert lib.emu_vg_norm(*shape, L, swt, do_app, flat.ctypes.data, C.byref(out)) == 0, (shape, swt, do_app)
            ref = prox.group_norm(bands, L, do_app)
            assert abs(np.longdouble(out.value) - ref) <= 2 * n * 2.0 ** -53 * ref, (shape, swt, do_app, out.value, ref)


def test_group_ops_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    for dtype in DTYPES:
        exe = str(tmp_path / ("emu_volume_group_san_%s" % np.dtype(dtype).name))
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_VOLUME_GROUP_MAIN",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
               "-static-libubsan"] + (["-DPDWT_DOUBLE"] if dtype == np.float64 else []) + ["-o", exe, SRC]
        subprocess.check_call(cmd)
        data, res = str(tmp_path / "records.bin"), str(tmp_path / "out.bin")
        rng = np.random.default_rng(43)
        want = []
        with open(data, "wb") as f:
            for shape, L, swt in SHAPES:
                flat = values(dtype, shape, L, swt, rng)
                bands = split(flat, shape, L, swt)
                for do_app in (0, 1):
                    betas = np.array(ops_ref.level_betas(26.0, L, 1, np.dtype(dtype).type), dtype=dtype)
                    f.write(np.array(list(shape) + [L, swt, do_app, flat.size], dtype=np.int64).tobytes())
                    f.write(betas.tobytes())
                    f.write(flat.tobytes())
                    out = prox.group_soft(bands, L, 26.0, do_app, 1)
                    want.append((shape, swt, do_app, prox.group_norm(bands, L, do_app), flat.size, out))
        r = subprocess.run([exe, data, res], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(want)
        got = np.fromfile(res, dtype=dtype)
        at = 0
        for line, (shape, swt, do_app, norm, n, out) in zip(lines, want):
            bad_walk, bad_soft, bad_norm, bits = line.split()
            assert int(bad_walk) == 0 and int(bad_soft) == 0 and int(bad_norm) == 0, (shape, swt, do_app, line)
            g = np.array([int(bits, 16)], dtype=np.uint64).view(np.float64)[0]
            assert abs(np.longdouble(g) - norm) <= 2 * n * 2.0 ** -53 * norm, (shape, swt, do_app, g, norm)
            for w in out:
                err = float(np.abs(got[at:at + w.size].astype(np.longdouble) - w.ravel().astype(np.longdouble)).max())
                assert err <= bound(w, dtype), (shape, swt, do_app, err)
                at += w.size
        assert at == got.size
