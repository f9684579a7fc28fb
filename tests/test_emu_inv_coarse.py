"""Index-math fuzz of dwt2_inv_coarse3_tile (three coarse inverse levels per launch, pypwt_amd/csrc/dwt2_inv_coarse_kernels.hpp)
through its CPU emulation (tests/cpu_emu/emu_inv_coarse.cpp, compiled here with its own g++ line into a temporary directory)
against the oracle.  CPU only; the same tile function is what the gfx950 kernel executes (tests/test_gpu_inv_coarse.py).

Sizes: multiples of (8, 32) up to 264 x 320 -- planes of one tile, of partial tiles on both axes, of regions that wrap on every side;
every candidate tile shape of the launcher; haar, db2, db3, db4 and a random 8-tap bank whose every tap counts (tests/tap_banks.py).
A shape whose staged regions do not fit the planes answers 1 and writes nothing: the predicate is part of what is fuzzed (every size
must be taken by the smallest shape unless a plane is smaller than that shape's region, and 32 x 32 by none)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tap_banks
from inv_coarse_geom import LEVELS, SHAPES, region_fits
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_emu", "emu_inv_coarse.cpp")
f32p = C.POINTER(C.c_float)


def P(a):
    return a.ctypes.data_as(f32p)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_inv_coarse") / "libemu_inv_coarse.so")
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unknown-pragmas",
                           "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.emu_dwt2_inv_coarse3.restype = C.c_int
    return lib


def _sizes():
    rng = np.random.default_rng(20261020)
    fixed = [(32, 32), (64, 96), (32, 256), (256, 32), (72, 288), (264, 320), (256, 256), (8, 32), (136, 160)]
    drawn = [(8 * int(rng.integers(1, 34)), 32 * int(rng.integers(1, 11))) for _ in range(6)]
    return fixed + drawn


def _filters():
    out = [(w,) + tuple(oracle.filters(w)) for w in ("haar", "db2", "db3", "db4")]
    out.append(("random8",) + tap_banks.bank(8, 77))
    return out


@pytest.mark.parametrize("filt", _filters(), ids=lambda f: f[0])
def test_emu_inv_coarse3_against_the_oracle(emu, filt):
    name, hlen, dlo, dhi, rlo, rhi = filt
    bank = None if name != "random8" else (hlen, dlo, dhi, rlo, rhi)
    took = 0
    for si, shape in enumerate(_sizes()):
        B = 3 if shape == (72, 288) else 1
        dims = [(shape[0] >> k, shape[1] >> k) for k in (1, 2, 3)]
        l1 = np.stack([oracle.hash_input((B,) + dims[0], 9100 + 10 * si + k, 2.0) - 1.0 for k in range(3)])  # H1,V1,D1
        l2 = np.stack([oracle.hash_input((B,) + dims[1], 9200 + 10 * si + k, 2.0) - 1.0 for k in range(3)])  # H2,V2,D2
        l3 = np.stack([oracle.hash_input((B,) + dims[2], 9300 + 10 * si + k, 2.0) - 1.0 for k in range(4)])  # A3,H3,V3,D3
        want = None
        for idx, (TX, TY) in SHAPES.items():
            out = np.full((B,) + shape, np.nan, dtype=np.float32)
            rc = emu.emu_dwt2_inv_coarse3(P(l1), P(l2), P(l3), B, shape[0], shape[1], P(rlo), P(rhi), hlen, idx, P(out))
            assert rc == (0 if region_fits(hlen, TX, TY, shape) else 1), (name, shape, idx, rc)
            if rc == 1:
                assert np.isnan(out).all(), (name, shape, idx, "a declined launch wrote")
                continue
            took += 1
            if want is None:
                want = []
                for b in range(B):
                    bands = [l3[0, b], l1[0, b], l1[1, b], l1[2, b], l2[0, b], l2[1, b], l2[2, b], l3[1, b], l3[2, b], l3[3, b]]
                    want.append(oracle.inverse(bands, shape, None if bank else name, LEVELS, ndim=2, filt=bank))
            for b in range(B):
                assert np.isfinite(out[b]).all(), (name, shape, idx)
                # the project's parity bound, 2e-6 (1 + L) of the largest sample (tests/test_gpu_dispatch.py), for these [-1, 1) bands
                tol = 2e-6 * (1 + LEVELS) * max(float(np.abs(want[b]).max()), 1.0)
                assert np.abs(out[b] - want[b]).max() <= tol, (name, shape, idx, float(np.abs(out[b] - want[b]).max()), tol)
        if shape == (32, 32):
            assert want is None, "32 x 32 is smaller than any tile's regions: declined by every shape"
    assert took >= 20
