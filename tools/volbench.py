#!/usr/bin/env python3
"""Times the 3D DWT of volumes (pypwt_amd.Wavelets3D) on the GPU.  Does not touch bench.py.

    python tools/volbench.py                       > profiles/volume_bench.txt     end-to-end times, device events
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/volbench.py --profile --case N
    python tools/volbench.py --summarize DIR --case N  > profiles/volume_rocprofv3_summary_<case>.txt

Default mode: per case forward, inverse and forward + soft threshold + inverse, each timed TWICE in the same call (the
spread) by two HIP events on the volume's stream around `--reps` calls (at least 50) after a warm-up of the same shapes.
Beside them the yardstick of the same run: the flat copy of the same bytes (pdwt_time_copy of a BatchedWavelets that holds the
level-1 slice stack) and the share of it that this plan's own level-1 2D kernel reaches (pdwt_time_level).  Gsamples/s and
the bytes moved per sample are computed from the shapes.

--ops: the operators on the coefficients of a volume (256^3 and 512^3 db4, three levels), each timed twice in the same call: the
global soft threshold and forward + soft + inverse as yardsticks, then band_stats, estimate_sigma, denoise, select_magnitude,
forward + keep_largest (keep_largest needs fresh coefficients every time; the forward of the same run is the line above it) and
forward + denoise + inverse.  Beside the times the rate at which the coefficients are READ: all 1 + 7 L sub-bands once for the
sweeps and the sums, the finest 'ddd' sub-band once per pass for estimate_sigma, the 7 L detail sub-bands once per pass for
select_magnitude; the keep sweep's own time is (forward + keep_largest) - forward - select_magnitude.

    python tools/volbench.py --ops                 > profiles/volume_opsbench.txt

--swt: the STATIONARY transform (Wavelets3D(..., do_swt=1)) of 256^3 db4 and 256^3 haar, three levels: forward, inverse and forward +
soft threshold + inverse by device events, as above.  The depth pass alone cannot be bracketed by events (it is one launch inside
the level), so its time per level comes from a kernel trace of the same shapes, with the yardstick IN THE SAME RUN: a flat copy
of the pass's algorithmic bytes (forward: 1 volume read + 2 written; inverse: 2 read + 1 written -- a copy of 1.5 volumes moves
the same 3 volumes of bytes).

    python tools/volbench.py --swt                                                           end-to-end times
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/volbench.py --swt --profile --case N
    python tools/volbench.py --swt --summarize DIR --case N                                  depth pass per level against the copy
    (the three outputs together are profiles/volume_swt_bench.txt)

--prox: the proximal operators (group_soft_threshold, group_norm, proj_linf, shrink, add_wavelet) on 256^3 and 512^3 db4 with three
levels, decimated; on 512 x 511 x 511 (div2 rounds up: its sub-bands have 256^3, 128^3, 64^3 values, all multiples of 4) and on
510^3 (255^3 values at level 1: the value-by-value path), decimated; and on 256^3 stationary.  Every line is timed twice by device
events after a warm-up.  In the same run, as yardsticks: the global soft_threshold sweep of the same volume and a flat copy of
the same number of values.  GB/s is the operator's ALGORITHMIC bytes over the faster time: the details read and written for the
two thresholds (8 B per detail value), read for the norm (4 B), all sub-bands read and written for proj_linf / shrink with the
approximation (8 B), two volumes read and one written for add_wavelet (12 B), 8 B per value for the copy.

    python tools/volbench.py --prox                > profiles/volume_proxbench.txt

--spin: circular shifts and cycle spinning (Wavelets3D.cycle_spin) on 256^3 and 512^3 db4 with three levels, every line timed twice
by device events after a warm-up: cycle_spin with 1 and with 8 lattice shifts and the soft threshold; in the same run the plain
decimated forward + soft + inverse and (256^3 only by default: 27 volumes) the stationary forward + soft + inverse; the in-place
circshift (the kernel plus the copy back).  The two kernels on their own, next to the flat copy of the same bytes in the same
process, come from tools/volshiftbench.hip, which this mode builds with hipcc when tools/bin/volshiftbench is missing or older
than its sources, on the same shapes and on 512 x 511 x 511 (value by value).

    python tools/volbench.py --spin                > profiles/volume_spin_bench.txt

--profile: a short run of ONE case with one level (so that every kernel name in the trace belongs to level 1) plus the copy and
the 2D level of the same bytes, for rocprofv3; --summarize reads the kernel trace of such a run and reports, per depth kernel,
its share of the copy next to the share the 2D level-1 kernel reaches.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, shape, wavelet, levels)
CASES = [("256^3 haar", (256, 256, 256), "haar", 3), ("256^3 db4", (256, 256, 256), "db4", 3), ("256^3 db20", (256, 256, 256), "db20", 3),
         ("512^3 haar", (512, 512, 512), "haar", 3), ("512^3 db4", (512, 512, 512), "db4", 3), ("512^3 db20", (512, 512, 512), "db20", 3),
         ("512x511x511 db4", (512, 511, 511), "db4", 3)]


def div2(n):
    return (n + (n & 1)) // 2


def bytes_per_sample(shape, levels, itemsize=4):
    """Bytes one direction of the composed transform moves per input sample: per level the depth pass reads A_{l-1} and writes
    the stack, the 2D level reads the stack and writes its four bands."""
    total, s = 0, shape
    for _ in range(levels):
        vol = s[0] * s[1] * s[2]
        stack = 2 * div2(s[0]) * s[1] * s[2]
        bands = 4 * 2 * div2(s[0]) * div2(s[1]) * div2(s[2])
        total += itemsize * (vol + stack + stack + bands)
        s = tuple(div2(n) for n in s)
    return total / float(shape[0] * shape[1] * shape[2])


class Events(object):
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time(self, stream, fn, reps, warmup):
        for _ in range(warmup):
            fn()
        assert self.hip.hipEventRecord(self.a, C.c_void_p(stream)) == 0
        for _ in range(reps):
            fn()
        assert self.hip.hipEventRecord(self.b, C.c_void_p(stream)) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value / reps


def make_volume(shape, wname, levels, do_swt=0):
    from pypwt_amd import Wavelets3D
    rng = np.random.default_rng(1)
    x = (rng.random(shape, dtype=np.float32) * np.float32(255.0))
    return Wavelets3D(x, wname, levels, do_swt=do_swt)


def variants(W):
    lib, h = W._lib, W._h

    def fwd():
        assert lib.pdwt_volume_forward(h) == 0

    def inv():  # the coefficients are declared current again in place (no copy, no device work), then the inverse runs
        assert lib.pdwt_volume_set_coeff(h, C.c_void_p(lib.pdwt_volume_coeff_ptr(h, 0)), 0, 1) == 0
        assert lib.pdwt_volume_inverse(h) == 0

    def denoise():
        assert lib.pdwt_volume_forward(h) == 0
        assert lib.pdwt_volume_soft_threshold(h, 10.0, 0, 0) == 0
        assert lib.pdwt_volume_inverse(h) == 0

    return [("forward", fwd, 1), ("inverse", inv, 1), ("fwd+soft+inv", denoise, 2)]


def yardstick(shape, wname, reps):
    """(copy ms, 2D level-1 forward ms, inverse ms) of the level-1 slice stack as a one-level batched 2D plan."""
    from pypwt_amd import BatchedWavelets
    B = BatchedWavelets(2 * div2(shape[0]), shape[1], shape[2], wname, 1)
    B.fill_hash(3)
    B.forward()
    elems = 2 * div2(shape[0]) * shape[1] * shape[2]
    out = (B.time_copy(elems, reps), B.time_level(1, False, reps), B.time_level(1, True, reps), B.time_copy(elems, reps))
    B.cleanup()
    return tuple(us / 1e3 for us in out)  # the plan reports microseconds


def run_bench(args):
    ev = Events()
    print("# volbench: 3D DWT end to end, fp32, %d calls per timing after %d warm-up calls; every variant timed twice" % (args.reps, args.warmup))
    print("# %-18s %-13s %10s %10s %12s %10s" % ("case", "variant", "ms (1st)", "ms (2nd)", "Gsamples/s", "B/sample"))
    for k, (name, shape, wname, levels) in enumerate(CASES):
        if args.case is not None and k != args.case:
            continue
        W = make_volume(shape, wname, levels)
        W.forward()
        n = shape[0] * shape[1] * shape[2]
        bps = bytes_per_sample(shape, W.levels)
        for vname, fn, directions in variants(W):
            t = [ev.time(W._stream(), fn, args.reps, args.warmup) for _ in range(2)]
            print("  %-18s %-13s %10.4f %10.4f %12.2f %10.1f" % (name, vname, t[0], t[1], directions * n / (min(t) * 1e6), bps * directions))
        W.cleanup()
        c0, f1, i1, c1 = yardstick(shape, wname, args.reps)
        print("  %-18s yardstick: copy of the level-1 stack %.4f / %.4f ms; 2D level-1 forward %.4f ms = %.2f of the copy, inverse %.4f ms = %.2f"
              % (name, c0, c1, f1, min(c0, c1) / f1, i1, min(c0, c1) / i1))
        sys.stdout.flush()


OPS_CASES = [("256^3 db4", (256, 256, 256), "db4", 3), ("512^3 db4", (512, 512, 512), "db4", 3)]


def run_ops(args):
    ev = Events()
    passes = 3  # fp32 keys: 11 + 10 + 10 bits
    print("# volbench --ops: operators on the coefficients of a volume, fp32, %d calls per timing after %d warm-up calls; every line timed twice"
          % (args.reps, args.warmup))
    print("# GB/s: coefficient bytes READ per call / the faster time (see the module docstring for what each operator reads)")
    print("# %-11s %-22s %10s %10s %10s" % ("case", "operator", "ms (1st)", "ms (2nd)", "GB/s read"))
    for k, (name, shape, wname, levels) in enumerate(OPS_CASES):
        if args.case is not None and k != args.case:
            continue
        W = make_volume(shape, wname, levels)
        W.forward()
        lib, h = W._lib, W._h
        sizes = [int(np.prod(W.band_shape(num))) for num in range(W.nbands)]
        n_all, n_det, n_noise = sum(sizes), sum(sizes[1:]), sizes[7]
        kk = n_det // 10

        def ok(rc):
            assert rc == 0, rc

        def soft():
            ok(lib.pdwt_volume_soft_threshold(h, 10.0, 0, 0))

        def fwd():
            ok(lib.pdwt_volume_forward(h))

        def inv():
            ok(lib.pdwt_volume_inverse(h))

        def fwd_soft_inv():
            fwd(), soft(), inv()

        def stats():
            ok(lib.pdwt_volume_band_stats_async(h, None))

        def sigma():
            ok(lib.pdwt_volume_estimate_sigma_async(h, 1, None))

        def denoise():
            ok(lib.pdwt_volume_denoise_async(h, 0, 0, None, 1))

        def select():
            ok(lib.pdwt_volume_select_magnitude_async(h, kk, 0, None, None))

        def fwd_keep():
            fwd()
            ok(lib.pdwt_volume_keep_largest_async(h, kk, 0))

        def fwd_denoise_inv():
            fwd(), denoise(), inv()

        rows = [("soft_threshold", soft, 4 * n_all), ("fwd+soft+inv", fwd_soft_inv, 0), ("forward", fwd, 0), ("band_stats", stats, 4 * n_all),
                ("estimate_sigma", sigma, 4 * passes * n_noise), ("select_magnitude K=N/10", select, 4 * passes * n_det),
                ("fwd+keep_largest K=N/10", fwd_keep, 0), ("denoise BayesShrink", denoise, 4 * (passes * n_noise + 2 * n_all)),
                ("fwd+denoise+inv", fwd_denoise_inv, 0)]
        got = {}
        for oname, fn, nbytes in rows:
            if oname in ("band_stats", "estimate_sigma", "select_magnitude K=N/10", "denoise BayesShrink", "soft_threshold"):
                fwd()  # dense coefficients under every operator that is timed on its own
            t = [ev.time(W._stream(), fn, args.reps, args.warmup) for _ in range(2)]
            got[oname] = min(t)
            rate = "%10.0f" % (nbytes / (min(t) * 1e6)) if nbytes else "%10s" % "-"
            print("  %-11s %-22s %10.4f %10.4f %s" % (name, oname, t[0], t[1], rate))
        keep = got["fwd+keep_largest K=N/10"] - got["forward"] - got["select_magnitude K=N/10"]
        print("  %-11s keep sweep alone: %.4f ms = %.0f GB/s read (and as much written where a value falls); N = %d, all coefficients %d"
              % (name, keep, 4 * n_det / (keep * 1e6) if keep > 0 else float("nan"), n_det, n_all))
        sys.stdout.flush()
        W.cleanup()


# (name, shape, wavelet, levels, stationary)
PROX_CASES = [("256^3 db4", (256, 256, 256), "db4", 3, 0), ("512^3 db4", (512, 512, 512), "db4", 3, 0),
              ("512x511x511 db4", (512, 511, 511), "db4", 3, 0), ("510^3 db4", (510, 510, 510), "db4", 3, 0),
              ("256^3 db4 swt", (256, 256, 256), "db4", 3, 1)]


def run_prox(args):
    from pypwt_amd import BatchedWavelets
    ev = Events()
    print("# volbench --prox: proximal operators on the coefficients of a volume, fp32, %d calls per timing after %d warm-up calls; every line timed twice"
          % (args.reps, args.warmup))
    print("# GB/s: algorithmic bytes per call / the faster time (see the module docstring); 'of soft': the operator's rate over the soft_threshold sweep's")
    print("# %-16s %-22s %10s %10s %10s %8s" % ("case", "operator", "ms (1st)", "ms (2nd)", "GB/s", "of soft"))
    for k, (name, shape, wname, levels, swt) in enumerate(PROX_CASES):
        if args.case is not None and k != args.case:
            continue
        W, W2 = make_volume(shape, wname, levels, swt), make_volume(shape, wname, levels, swt)
        W.forward(), W2.forward()
        lib, h = W._lib, W._h
        sizes = [int(np.prod(W.band_shape(num))) for num in range(W.nbands)]
        n_all, n_det = sum(sizes), sum(sizes[1:])
        n_l = [sizes[1 + 7 * l] for l in range(W.levels)]

        def ok(rc):
            assert rc == 0, rc

        def soft():
            ok(lib.pdwt_volume_soft_threshold(h, 10.0, 0, 0))

        def group():
            ok(lib.pdwt_volume_group_soft_threshold(h, 10.0, 0, 0))

        def norm():
            ok(lib.pdwt_volume_group_norm_async(h, 0, None, None))

        def linf():
            ok(lib.pdwt_volume_proj_linf(h, 10.0, 1))

        def shrink():
            ok(lib.pdwt_volume_shrink(h, 0.001, 1))

        def axpy():
            ok(lib.pdwt_volume_add_wavelet(h, W2._h, 0.001))

        rows = [("soft_threshold", soft, 8 * n_det), ("group_soft_threshold", group, 8 * n_det), ("group_norm", norm, 4 * n_det),
                ("proj_linf", linf, 8 * n_all), ("shrink", shrink, 8 * n_all), ("add_wavelet", axpy, 12 * n_all)]
        rate = {}
        for oname, fn, nbytes in rows:
            ok(lib.pdwt_volume_forward(h))  # dense coefficients under every operator
            t = [ev.time(W._stream(), fn, args.reps, args.warmup) for _ in range(2)]
            rate[oname] = nbytes / (min(t) * 1e6)
            print("  %-16s %-22s %10.4f %10.4f %10.0f %8.2f" % (name, oname, t[0], t[1], rate[oname], rate[oname] / rate["soft_threshold"]))
        W.cleanup(), W2.cleanup()
        B = BatchedWavelets(n_all // (shape[1] * shape[2]) + 1, shape[1], shape[2], "haar", 1)
        B.fill_hash(3)
        elems = min(n_all, B.copy_capacity())
        t = [B.time_copy(elems, args.reps) / 1e3 for _ in range(2)]
        B.cleanup()
        print("  %-16s %-22s %10.4f %10.4f %10.0f %8.2f" % (name, "flat copy, %d values" % elems, t[0], t[1], 8 * elems / (min(t) * 1e6),
                                                            8 * elems / (min(t) * 1e6) / rate["soft_threshold"]))
        print("  %-16s positions per level %s (%s); group_soft_threshold reaches %.2f of the soft_threshold sweep"
              % (name, n_l, ", ".join("groups of four" if n % 4 == 0 else "value by value" for n in n_l),
                 rate["group_soft_threshold"] / rate["soft_threshold"]))
        sys.stdout.flush()


SWT_CASES = [("256^3 db4", (256, 256, 256), "db4", 3), ("256^3 haar", (256, 256, 256), "haar", 3)]


def run_swt(args):
    ev = Events()
    print("# volbench --swt: stationary 3D transform end to end, fp32, %d calls per timing after %d warm-up calls; every variant timed twice"
          % (args.reps, args.warmup))
    print("# %-12s %-13s %10s %10s %12s   %s" % ("case", "variant", "ms (1st)", "ms (2nd)", "Gsamples/s", "depth schedule (width, seg fwd, seg inv) per level"))
    for k, (name, shape, wname, levels) in enumerate(SWT_CASES):
        if args.case is not None and k != args.case:
            continue
        W = make_volume(shape, wname, levels, do_swt=1)
        W.forward()
        n = shape[0] * shape[1] * shape[2]
        sched = [W.depth_schedule(l) for l in range(1, W.levels + 1)]
        for vname, fn, directions in variants(W):
            t = [ev.time(W._stream(), fn, args.reps, args.warmup) for _ in range(2)]
            print("  %-12s %-13s %10.4f %10.4f %12.2f   %s" % (name, vname, t[0], t[1], directions * n / (min(t) * 1e6), sched))
        W.cleanup()
        sys.stdout.flush()


def swt_copy_yardstick(shape, reps):
    """A flat copy that moves the depth pass's algorithmic bytes (3 volumes): 1.5 volumes read, 1.5 written."""
    from pypwt_amd import BatchedWavelets
    B = BatchedWavelets(shape[0] * 3 // 2, shape[1], shape[2], "haar", 1)
    B.fill_hash(3)
    elems = (shape[0] * 3 // 2) * shape[1] * shape[2]
    us = B.time_copy(elems, reps)
    B.cleanup()
    return elems, us


def swt_case(args):
    if args.case is None or not 0 <= args.case < len(SWT_CASES):
        raise SystemExit("--swt --profile / --summarize need --case N with N in 0 .. %d: %s" % (len(SWT_CASES) - 1, [c[0] for c in SWT_CASES]))
    return SWT_CASES[args.case]


def run_swt_profile(args):
    name, shape, wname, levels = swt_case(args)
    W = make_volume(shape, wname, levels, do_swt=1)
    vs = dict((v[0], v[1]) for v in variants(W))
    for _ in range(args.reps):
        vs["forward"]()
        vs["inverse"]()
    W.synchronize()
    W.cleanup()
    print("profiled", name, "stationary, levels=%d" % levels, swt_copy_yardstick(shape, args.reps))


def run_swt_summarize(args):
    name, shape, wname, levels = swt_case(args)
    files = glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + args.summarize)
    rows = []
    for f in files:
        for row in csv.DictReader(open(f)):
            k = re.sub(r"^void |pdwt::|\(.*$", "", row["Kernel_Name"])
            rows.append((int(row["Start_Timestamp"]), k, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0))
    rows.sort()
    median = lambda v: sorted(v)[len(v) // 2]
    copy = [d for _, k, d in rows if k.startswith("copy_kernel")]
    if not copy:
        raise SystemExit("no copy_kernel in the trace")
    vol_bytes = 4.0 * shape[0] * shape[1] * shape[2]
    print("# %s stationary, %d levels: kernel trace, median us per launch; the depth pass moves 3 volumes = %.1f MB" % (name, levels, 3 * vol_bytes / 1e6))
    print("  %-44s %9.2f us  %7.0f GB/s" % ("copy_kernel of the same bytes (n=%d)" % len(copy), median(copy), 3 * vol_bytes / (median(copy) * 1e3)))
    for direction in ("fwd", "inv"):
        d = [(k, t) for _, k, t in rows if k.startswith("swt3_depth_%s_kernel" % direction)]
        if not d or len(d) % levels:
            raise SystemExit("expected a multiple of %d swt3_depth_%s launches, found %d" % (levels, direction, len(d)))
        for i in range(levels):  # launches come level by level: forward 1 .. L, inverse L .. 1
            level = i + 1 if direction == "fwd" else levels - i
            t = [x[1] for x in d[i::levels]]
            print("  %-44s %9.2f us  %7.0f GB/s  %.2f of the copy" % ("%s level %d (f = %d, n=%d)" % (d[i][0], level, 1 << (level - 1), len(t)), median(t),
                                                                     3 * vol_bytes / (median(t) * 1e3), median(copy) / median(t)))
    other = {}
    for _, k, t in rows:
        if not k.startswith("swt3_depth") and not k.startswith("copy_kernel"):
            other.setdefault(k, []).append(t)
    for k, v in sorted(other.items(), key=lambda kv: -sum(kv[1])):
        print("  %-60s n=%4d median %9.2f us" % (k[:60], len(v), median(v)))


SPIN_CASES = [("256^3 db4", (256, 256, 256), "db4", 3, True), ("512^3 db4", (512, 512, 512), "db4", 3, False)]
SPIN_KERNEL_SHAPES = [(256, 256, 256), (512, 512, 512), (512, 511, 511)]


def shift_bench_program():
    """tools/bin/volshiftbench, built from tools/volshiftbench.hip when it is missing or older than what it includes."""
    import shutil
    import subprocess
    src = os.path.join(ROOT, "tools", "volshiftbench.hip")
    csrc = os.path.join(ROOT, "pypwt_amd", "csrc")
    exe = os.path.join(ROOT, "tools", "bin", "volshiftbench")
    deps = [src, os.path.join(csrc, "volume_shift_kernels.hpp"), os.path.join(csrc, "kernels_common.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", csrc, src, "-o", exe])
    return exe


def run_spin(args):
    import subprocess
    from pypwt_amd.volume import spin_footprint, spin_lattice, volume_layout_swt
    ev = Events()
    print("# volbench --spin: cycle spinning of a volume, fp32, %d calls per timing after %d warm-up calls; every line timed twice" % (args.reps, args.warmup))
    print("# %-11s %-34s %10s %10s %9s %9s" % ("case", "what", "ms (1st)", "ms (2nd)", "x 1 shift", "x swt"))
    for k, (name, shape, wname, levels, with_swt) in enumerate(SPIN_CASES):
        if args.case is not None and k != args.case:
            continue
        W = make_volume(shape, wname, levels)
        lib, h = W._lib, W._h
        lat = np.ascontiguousarray(spin_lattice(8))
        sh = lat.ctypes.data_as(C.POINTER(C.c_int))

        def ok(rc):
            assert rc == 0, rc

        def plain():
            ok(lib.pdwt_volume_forward(h)), ok(lib.pdwt_volume_soft_threshold(h, 10.0, 0, 0)), ok(lib.pdwt_volume_inverse(h))

        def spin(nshifts):
            return lambda: ok(lib.pdwt_volume_cycle_spin_async(h, nshifts, sh, 0, 10.0, 0, 0, -1, None, 1))

        def inplace():
            ok(lib.pdwt_volume_circshift(h, 1, 2, 4))

        got = {}
        rows = [("forward + soft + inverse", plain), ("cycle_spin, 1 shift, soft", spin(1)), ("cycle_spin, 8 shifts, soft", spin(8)),
                ("circshift in place (1, 2, 4)", inplace)]
        for what, fn in rows:
            t = [ev.time(W._stream(), fn, args.reps, args.warmup) for _ in range(2)]
            got[what] = (t[0], t[1])
        W.cleanup()
        if with_swt:
            S = make_volume(shape, wname, levels, do_swt=1)
            fn = dict((v[0], v[1]) for v in variants(S))["fwd+soft+inv"]
            t = [ev.time(S._stream(), fn, args.reps, args.warmup) for _ in range(2)]
            got["stationary forward + soft + inverse"] = (t[0], t[1])
            S.cleanup()
        one = min(got["cycle_spin, 1 shift, soft"])
        swt = min(got["stationary forward + soft + inverse"]) if with_swt else None
        for what, t in got.items():
            print("  %-11s %-34s %10.4f %10.4f %9.2f %9s" % (name, what, t[0], t[1], min(t) / one, "%9.2f" % (min(t) / swt) if swt else "-"))
        vol = 4.0 * shape[0] * shape[1] * shape[2]
        print("  %-11s device memory: decimated handle about 3.3 volumes + cycle_spin %.2f volumes; stationary handle %.1f volumes"
              % (name, spin_footprint(shape, np.float32) / vol, volume_layout_swt(shape, wname, levels)[1] / vol))
        sys.stdout.flush()
    if args.case is None:
        exe = shift_bench_program()
        print("# the two kernels on their own (tools/volshiftbench.hip): ms (1st), ms (2nd), GB/s of the bytes moved, share of the same-run flat copy")
        sys.stdout.flush()
        for shape in SPIN_KERNEL_SHAPES:
            subprocess.check_call([exe] + [str(n) for n in shape] + [str(args.reps), str(args.warmup)])


def run_profile(args):
    name, shape, wname, _ = CASES[args.case]
    W = make_volume(shape, wname, 1)
    vs = dict((v[0], v[1]) for v in variants(W))
    for _ in range(args.reps):
        vs["forward"]()
        vs["inverse"]()
    W.synchronize()
    W.cleanup()
    print("profiled", name, "levels=1", yardstick(shape, wname, args.reps))


def run_summarize(args):
    name, shape, wname, _ = CASES[args.case]
    files = glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + args.summarize)
    dur = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            k = re.sub(r"^void |pdwt::|\(.*$", "", row["Kernel_Name"])
            dur.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    print("# %s, one level: kernel trace, us per launch (n, mean, median, min)" % name)
    med = {}
    for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        v = sorted(v)
        med[k] = v[len(v) // 2]
        print("  %-50s n=%4d mean=%9.2f med=%9.2f min=%9.2f" % (k, len(v), sum(v) / len(v), med[k], v[0]))
    copy = [m for k, m in med.items() if k.startswith("copy_kernel")]
    if not copy:
        raise SystemExit("no copy_kernel in the trace")
    copy = min(copy)
    print("# share of the flat copy of the same bytes (copy median %.2f us): copy / kernel" % copy)
    for k, m in sorted(med.items()):
        if k.startswith("dwt3_depth") or k.startswith("dwt2_"):
            print("  %-50s %.2f" % (k, copy / m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--ops", action="store_true")
    ap.add_argument("--swt", action="store_true")
    ap.add_argument("--prox", action="store_true")
    ap.add_argument("--spin", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--list", action="store_true")
    args = ap.parse_args()
    if args.list:
        for k, c in enumerate(CASES):
            print(k, c, "bytes/sample per direction %.1f" % bytes_per_sample(c[1], c[3]))
        return
    if args.prox:
        run_prox(args)
    elif args.spin:
        run_spin(args)
    elif args.swt:
        if args.summarize:
            run_swt_summarize(args)
        elif args.profile:
            run_swt_profile(args)
        else:
            run_swt(args)
    elif args.summarize:
        run_summarize(args)
    elif args.profile:
        run_profile(args)
    elif args.ops:
        run_ops(args)
    else:
        run_bench(args)


if __name__ == "__main__":
    main()
