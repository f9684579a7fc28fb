"""The 2D kernel families that load 16-byte groups at 4-byte alignment on planes of any width, under the address and
undefined-behaviour sanitizers.

tests/cpu_emu/emu_san.cpp is built once per family (only that family's kernel headers: all of emu_kernels.cpp under the
sanitizers compiles for longer than a test may) as a stand-alone program.  It reads the cases from a file, gives every input
plane, output plane and filter array a heap block of exactly its size, sizes the emulated LDS to the geometry's element
(-DEMU_SLACK=0), fills the outputs with NaN, runs the family's emu_* entry point and writes the outputs to a file.  Here the
program is compiled, run once with ASAN_OPTIONS=detect_leaks=1 and UBSAN_OPTIONS=halt_on_error=1, must exit with status 0,
and its outputs must equal, bit for bit, what the unsanitised shared library of tests/emu_util.py computes on the same
arrays -- whose parity with the oracle tests/test_emu_tiles.py asserts.  Nothing sanitised is loaded into python.

A parity test cannot see what these see: a load of samples the staging throws away leaves every result right.  The
one-launch SWT levels did that (a 16-byte group behind the needed window of a staged row, begun inside the row and ended
behind it: behind the plane on the last row of the last image) until swt_stage_col; and the last NEEDED group did the same
where a strip's window ended within three samples of the row end (swt_stage_pad laid the groups out from column 0 there).

A combination the emulation's entry point declines (status -2: a chain of rows shorter than one step, a width the family does
not take) has nothing to run; each test counts them and states which they are.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from emu_san_util import IN, OUT, SAN, compile_programs
from emu_san_util import nan as _nan
from emu_san_util import plane as _plane
from emu_san_util import run as _run
from emu_util import EMU_DIR, P, lib
from oracle import oracle

# family -> what selects it and the filter lengths / dilations its program instantiates (the cases below use no other)
FAMILIES = {
    "fwdstream": ["-DEMU_SAN_FWDSTREAM", "-DEMU_FWDSTREAM_HLENS(X)=X(6) X(8) X(20)", "-DEMU_FWDSTREAM_DILATIONS(Y,h)=Y(h,1) Y(h,2) Y(h,4)"],
    "invstream": ["-DEMU_SAN_INVSTREAM", "-DEMU_INVSTREAM_HLENS(X)=X(6) X(8) X(16)", "-DEMU_INVSTREAM_DILATIONS(Y,h)=Y(h,1) Y(h,2) Y(h,4)"],
    "fused": ["-DEMU_SAN_FUSED"],
    "fast": ["-DEMU_SAN_FAST", "-DEMU_FAST_HLENS(X)=X(2) X(4) X(8)"],
    "split": ["-DEMU_SAN_SPLIT", "-DEMU_SPLIT_HLENS(X)=X(10) X(20)"],
    "long": ["-DEMU_SAN_LONG", "-DEMU_LONG_HLENS(X)=X(10) X(20) X(40)"],
}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """Every family's program, compiled side by side (emu_san_util.compile_programs); family -> a function returning its path."""
    get, finish = compile_programs(tmp_path_factory.mktemp("emu_san"), FAMILIES)
    yield get
    finish()


def _widths(hlen, f):
    """The narrowest row that is not whole 16-B groups and the one-launch SWT launchers accept, and the next seven: every residue mod 4."""
    w0 = 64 + (hlen - 1) * f + 4
    return list(range(w0, w0 + 8))


def _swt_stream_grid(wnames):
    """(wname, hlen, level, Nr, Nc, B, seg) of the one-launch SWT levels.  Rows: 64, 67 (no dilation above 1 divides it: one chain
    of all rows), and 128 where chains of 64 rows / dilation are shorter than the launch's step."""
    grid = []
    for wname in wnames:
        hlen = oracle.filters(wname)[0]
        for level in (1, 2, 3):
            for Nc in _widths(hlen, 1 << (level - 1)):
                for Nr in (64, 67) + ((128,) if level == 3 else ()):
                    for B in (1, 2):
                        for seg in (0, 32):
                            grid.append((wname, hlen, level, Nr, Nc, B, seg))
        # ... and the widths at which the window of strip 1 ends at the row end or up to 3 samples in front of it (its columns run to
        # 128 + f hlen / 2): groups laid out from column 0 had the last needed one across the end (6 taps: 131 columns)
        for level in (1, 2, 3):
            f = 1 << (level - 1)
            for Nc in range(128 + f * hlen // 2, 128 + f * hlen // 2 + 4):
                if Nc >= _widths(hlen, f)[0]:
                    grid += [(wname, hlen, level, 67, Nc, B, 0) for B in (1, 2)]
    # the shapes of the first finding (8 taps, dilation 1: strip 1 of 64 x 133 stages columns 58 ... 135) and whole groups beside them
    grid += [("db4", 8, 1, 64, Nc, B, seg) for Nc in (133, 134, 135, 136) for B in (1, 2) for seg in (0, 32)]
    grid += [("sym8", 16, 2, 66, 161, 1, 0)] if "sym8" in wnames else []
    return grid


def test_swt_forward_level_in_one_launch_under_sanitizers(programs, tmp_path):
    """swt_fwdstream_kernels.hpp: 6, 8 and 20 taps, dilations 1, 2 and 4, the eight narrowest widths of each, one and two images,
    one and several segments per chain.  Declined: 64 rows at dilation 4 (chains of 16 rows, a step is 32)."""
    L = lib()
    cases, declined = [], []
    for wname, hlen, level, Nr, Nc, B, seg in _swt_stream_grid(("db3", "db4", "db10")):
        _, dlo, dhi, _, _ = oracle.filters(wname)
        x = _plane((B, Nr, Nc), 7100 + level)
        outs = [_nan((B, Nr, Nc)) for _ in range(4)]
        rc = L.emu_swt2_fwdstream(P(x), B, Nr, Nc, level, P(dlo), P(dhi), hlen, seg, *[P(o) for o in outs])
        if rc == -2:
            declined.append((level, Nr))
            continue
        assert rc == 0, (wname, level, Nr, Nc, rc)
        cases.append(([B, Nr, Nc, level, hlen, seg], [], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
    assert set(declined) == {(3, 64)}
    assert any(c[0][:5] == [1, 64, 133, 1, 8] for c in cases) and len(cases) >= 3 * (3 * 8 * 2) * 4
    _run(programs("fwdstream"), tmp_path, cases)


def test_swt_inverse_level_in_one_launch_under_sanitizers(programs, tmp_path):
    """swt_invstream_kernels.hpp: the same grid with 6, 8 and 16 taps, with and without the pending soft threshold.  Nothing is
    declined: its steps at dilation 4 are 16 rows."""
    L = lib()
    cases = []
    for wname, hlen, level, Nr, Nc, B, seg in _swt_stream_grid(("db3", "db4", "sym8")):
        _, _, _, rlo, rhi = oracle.filters(wname)
        bands = [_plane((B, Nr, Nc), 7200 + 4 * level + k, signed=True) for k in range(4)]
        for beta in (0.0, 0.25):
            rec = _nan((B, Nr, Nc))
            rc = L.emu_swt2_invstream(*[P(b) for b in bands], B, Nr, Nc, level, P(rlo), P(rhi), hlen, C.c_float(beta), seg, P(rec))
            assert rc == 0, (wname, level, Nr, Nc, rc)
            cases.append(([B, Nr, Nc, level, hlen, seg], [beta], [(b, IN) for b in bands] + [(rlo, IN), (rhi, IN), (rec, OUT)]))
    assert any(c[0][:5] == [1, 66, 161, 2, 16] for c in cases)
    _run(programs("invstream"), tmp_path, cases)


def _fused_case(L, taps, B, Nr, Nc, K, f0, seg, inverse, cpl, wname, with_beta):
    _, dlo, dhi, rlo, rhi = oracle.filters(wname)
    lo, hi = (rlo, rhi) if inverse & 1 else (dlo, dhi)
    beta = np.array([0.3, 0.2, 0.1][:K], dtype=np.float32) if with_beta else None
    a = _plane((B, Nr, Nc), 7300 + K, signed=True)
    if inverse & 1:
        det, out = _plane((3 * K, B, Nr, Nc), 7310 + K, signed=True), _nan((B, Nr, Nc))
        bufs = [(a, IN), (det, IN), (out, OUT)]
    else:
        det, out = _nan((3 * K, B, Nr, Nc)), _nan((B, Nr, Nc))
        bufs = [(a, IN), (det, OUT), (out, OUT)]
    if taps == 2:
        rc = L.emu_swt2_fused(P(a), P(det), P(out), B, Nr, Nc, K, f0, seg, P(lo), P(hi), P(beta) if with_beta else None, inverse, cpl)
    else:
        rc = L.emu_swt4_fused(P(a), P(det), P(out), B, Nr, Nc, f0, seg, P(lo), P(hi), P(beta) if with_beta else None, inverse)
    return rc, ([taps, B, Nr, Nc, K, f0, seg, inverse, cpl], [], bufs + [(lo, IN), (hi, IN), (beta, IN)])


def test_swt_fused_2tap_groups_on_any_size_under_sanitizers(programs, tmp_path):
    """swt2_fused_kernels.hpp, the GEN instantiations (forced on the aligned widths too): widths 256 ... 263, two and three levels,
    first dilation 1 and 8, forward and inverse, 16-B and 8-B lanes of the inverse, row counts the dilation does and does not divide."""
    L = lib()
    cases = []
    for Nc in range(256, 264):
        for K in (2, 3):
            for f0 in (1, 8):
                for Nr, B in ((64, 1), (67, 2)):
                    for inverse, cpl, with_beta in ((0, 4, False), (1, 4, True), (1, 2, False)):
                        rc, case = _fused_case(L, 2, B, Nr, Nc, K, f0, 8, inverse, 8 + cpl, "haar", with_beta)
                        assert rc == 0, (Nc, K, f0, Nr, inverse, cpl, rc)
                        cases.append(case)
    _run(programs("fused"), tmp_path, cases)


def test_swt_fused_4tap_pairs_on_any_size_under_sanitizers(programs, tmp_path):
    """swt2_fused4_kernels.hpp: widths 256 ... 263 (GEN, forced with inverse + 2 where the size is aligned) and 64 ... 71 (the
    aligned instantiations), first dilation 1 and 4, rows 32 and 35.  Declined: below 256 columns every size the aligned
    instantiations cannot take (a width that is not whole groups, 35 rows at dilation 4, GEN forced)."""
    L = lib()
    cases, declined = [], 0
    for Nc in list(range(256, 264)) + list(range(64, 72)):
        for f0 in (1, 4):
            for Nr in (32, 35):
                for inverse in (0, 1, 2, 3):
                    rc, case = _fused_case(L, 4, 1, Nr, Nc, 2, f0, 8, inverse, 0, "db2", bool(inverse & 1))
                    general = Nc % 4 != 0 or Nr % f0 != 0 or inverse & 2
                    assert rc == (-2 if Nc < 256 and general else 0), (Nc, f0, Nr, inverse, rc)
                    if rc == 0:
                        cases.append(case)
                    else:
                        declined += 1
    assert len(cases) == 8 * 2 * 2 * 4 + 2 * 3 * 2 and declined == 8 * 2 * 2 * 4 - 2 * 3 * 2
    _run(programs("fused"), tmp_path, cases)


def test_dwt2_fast_tiles_unaligned_staging_under_sanitizers(programs, tmp_path):
    """dwt2_fast_kernels.hpp, forward and inverse: 2, 4 and 8 taps, widths 61 ... 70, 33 and 34 rows, every tile shape (the
    staging clamps what lies past the end of a tile)."""
    L = lib()
    cases = []
    for wname in ("haar", "db2", "db4"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for Nc in range(61, 71):
            for Nr in (33, 34):
                r2, c2 = (Nr + 1) // 2, (Nc + 1) // 2
                x = _plane((1, Nr, Nc), 7400)
                bands = [_plane((1, r2, c2), 7410 + k, signed=True) for k in range(4)]
                for tile in (0, 1, 2):
                    outs = [_nan((1, r2, c2)) for _ in range(4)]
                    assert L.emu_dwt2_fwd_fast(P(x), 1, Nr, Nc, P(dlo), P(dhi), hlen, tile, *[P(o) for o in outs]) == 0
                    cases.append(([0, 1, Nr, Nc, hlen, tile], [], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
                    rec = _nan((1, Nr, Nc))
                    assert L.emu_dwt2_inv_fast(*[P(b) for b in bands], 1, r2, c2, Nr, Nc, P(rlo), P(rhi), hlen, tile, P(rec)) == 0
                    cases.append(([1, 1, Nr, Nc, hlen, tile], [], [(b, IN) for b in bands] + [(rlo, IN), (rhi, IN), (rec, OUT)]))
    _run(programs("fast"), tmp_path, cases)


def test_swt_column_pass_as_a_strip_walk_under_sanitizers(programs, tmp_path, monkeypatch):
    """swt_colstream_kernels.hpp through emu_swt2_split with EMU_SPLIT_COLSTREAM: 10 and 20 taps, dilations 1, 2 and 4, both
    directions, the pending soft threshold, one and several segments; the program fails a case whose column pass did not take the
    strip kernels.  Declined: every width that is not whole 16-B groups (65 ... 67, 69 ... 71) -- the two-launch level takes none."""
    L = lib()
    monkeypatch.setenv("EMU_SPLIT_COLSTREAM", "1")
    cases, declined = [], set()
    for wname in ("db5", "db10"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for (Nr, level, B) in ((64, 1, 2), (97, 1, 1), (135, 2, 1), (160, 3, 1)):
            for Nc in list(range(64, 72)) + [136, 200]:
                for seg in (0, 32):
                    if seg:
                        monkeypatch.setenv("EMU_COLSTREAM_SEG", str(seg))
                    else:
                        monkeypatch.delenv("EMU_COLSTREAM_SEG", raising=False)
                    x = _plane((B, Nr, Nc), 7500 + level)
                    outs = [_nan((B, Nr, Nc)) for _ in range(4)]
                    before = L.emu_colstream_runs()
                    rc = L.emu_swt2_split(0, P(x), B, Nr, Nc, level, P(dlo), P(dhi), hlen, C.c_float(0.0), *[P(o) for o in outs])
                    if rc == -2:
                        declined.add(Nc)
                        continue
                    assert rc == 0 and L.emu_colstream_runs() == before + 1, (wname, Nr, Nc, level)
                    cases.append(([0, B, Nr, Nc, level, hlen, seg], [0.0], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
                    bands = [_plane((B, Nr, Nc), 7510 + 4 * level + k, signed=True) for k in range(4)]
                    for beta in (0.0, 0.25):
                        rec = _nan((B, Nr, Nc))
                        assert L.emu_swt2_split(1, P(rec), B, Nr, Nc, level, P(rlo), P(rhi), hlen, C.c_float(beta), *[P(b) for b in bands]) == 0
                        cases.append(([1, B, Nr, Nc, level, hlen, seg], [beta], [(rec, OUT), (rlo, IN), (rhi, IN)] + [(b, IN) for b in bands]))
    assert declined == {65, 66, 67, 69, 70, 71}
    _run(programs("split"), tmp_path, cases)


def test_dwt2_long_filter_strip_walks_under_sanitizers(programs, tmp_path):
    """dwt2_long_kernels.hpp, forward and inverse: 10, 20 and 40 taps, every launch shape of the emulation, ragged last strips and
    steps, one segment and several, one and two images, planes narrower than the filter (the periodic index wraps more than once)."""
    L = lib()
    cases = []
    for wname in ("db5", "db10", "db20"):
        hlen, dlo, dhi, rlo, rhi = oracle.filters(wname)
        for B, Nr, Nc, seg in ((1, 64, 72, 0), (2, 66, 136, 16), (1, 96, 264, 8), (1, 32, 16, 0), (1, 130, 40, 16)):
            r2, c2 = Nr // 2, Nc // 2
            assert c2 % 4 == 0
            x = _plane((B, Nr, Nc), 7600)
            bands = [_plane((B, r2, c2), 7610 + k, signed=True) for k in range(4)]
            for shape in range(4):
                outs = [_nan((B, r2, c2)) for _ in range(4)]
                assert L.emu_dwt2_fwd_long(P(x), B, Nr, Nc, P(dlo), P(dhi), hlen, seg, shape, *[P(o) for o in outs]) == 0
                cases.append(([0, B, Nr, Nc, hlen, seg, shape], [], [(x, IN), (dlo, IN), (dhi, IN)] + [(o, OUT) for o in outs]))
                rec = _nan((B, Nr, Nc))
                assert L.emu_dwt2_inv_long(*[P(b) for b in bands], B, r2, c2, Nr, Nc, P(rlo), P(rhi), hlen, seg, shape, P(rec)) == 0
                cases.append(([1, B, Nr, Nc, hlen, seg, shape], [], [(b, IN) for b in bands] + [(rlo, IN), (rhi, IN), (rec, OUT)]))
    _run(programs("long"), tmp_path, cases)


def test_inverse_coarse_program_under_sanitizers(tmp_path):
    """tests/cpu_emu/emu_inv_coarse.cpp as its own program (-DEMU_INV_COARSE_MAIN): every tile shape and filter length of the
    three-level inverse over planes with interior, border and partial tiles, the LDS sized exactly, each result against a synthesis
    written out plainly in the program."""
    exe = str(tmp_path / "emu_inv_coarse_san")
    san = [a for a in SAN if a != "-DEMU_SLACK=0"]
    subprocess.check_call(san + ["-DEMU_INV_COARSE_MAIN", "-o", exe, os.path.join(EMU_DIR, "emu_inv_coarse.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    runs, declined, failures = [int(t) for t in r.stdout.split() if t.isdigit()][-3:]
    assert runs > 0 and declined > 0 and failures == 0, r.stdout[-300:]
