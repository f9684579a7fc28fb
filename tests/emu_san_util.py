"""What tests/test_emu_sanitized.py and tests/test_emu_sanitized_more.py share: the compile line of tests/cpu_emu/emu_san.cpp, the
record format of its input, one run of a family's program against the unsanitised shared library's outputs."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from emu_util import EMU_DIR
from oracle import oracle

SRC = os.path.join(EMU_DIR, "emu_san.cpp")
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DPDWT_CPU_EMU", "-DEMU_SLACK=0",
       "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
       "-static-libubsan"]
IN, OUT = 0, 1


def compile_programs(d, families):
    """Starts the compile of every family's program (family -> flags) into directory d, no more compilers at once than this process
    may use CPUs, 16 at the most.  Returns (get, finish): get(family) waits for that program and returns its path."""
    jobs = max(1, min(16, len(os.sched_getaffinity(0))))
    pool = ThreadPoolExecutor(max_workers=jobs)

    def build(family):
        return subprocess.run(SAN + families[family] + ["-o", str(d / family), SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    futures = {f: pool.submit(build, f) for f in families}

    def get(family):
        r = futures[family].result()
        assert r.returncode == 0, r.stdout[-3000:]
        return str(d / family)

    def finish():
        pool.shutdown(wait=True)
        _inputs.clear()
    return get, finish


def record(f, ints, flts, bufs):
    """One record of emu_san.cpp's input; bufs: (array or None, IN / OUT)."""
    f.write(np.array([len(ints)] + list(ints), dtype=np.int64).tobytes())
    f.write(np.array([len(flts)], dtype=np.int64).tobytes() + np.array(flts, dtype=np.float32).tobytes())
    f.write(np.array([len(bufs)], dtype=np.int64).tobytes())
    for a, kind in bufs:
        f.write(np.array([-1 if a is None else a.size, kind], dtype=np.int64).tobytes())
        if a is not None and kind == IN:
            assert a.dtype == np.float32 and a.flags.c_contiguous
            f.write(a.tobytes())


def run(exe, tmp_path, cases):
    """cases: (ints, flts, bufs) with the OUT arrays already filled by the unsanitised library.  Runs the program once."""
    data, res = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(data, "wb") as f:
        for ints, flts, bufs in cases:
            record(f, ints, flts, bufs)
    env = {k: v for k, v in os.environ.items() if k not in ("EMU_SPLIT_COLSTREAM", "EMU_COLSTREAM_SEG", "EMU_SPLIT_DIRECT")}
    r = subprocess.run([exe, data, res], capture_output=True, text=True, timeout=900,
                       env=dict(env, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert int(r.stdout.split()[-1]) == len(cases)
    want = np.concatenate([a.ravel() for _, _, bufs in cases for a, kind in bufs if kind == OUT and a is not None])
    assert not np.isnan(want).any()  # the library wrote every output element
    got = np.fromfile(res, dtype=np.float32)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


_inputs = {}


def plane(shape, seed, signed=False):
    """oracle.hash_input, as in tests/test_emu_tiles.py (coefficients: in [-1, 1)); computed once per (shape, seed)."""
    key = (shape, seed, signed)
    if key not in _inputs:
        x = oracle.hash_input(shape, seed, 2.0) - 1.0 if signed else oracle.hash_input(shape, seed)
        _inputs[key] = np.ascontiguousarray(x, dtype=np.float32)
    return _inputs[key]


def nan(shape):
    return np.full(shape, np.nan, dtype=np.float32)
