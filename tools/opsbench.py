#!/usr/bin/env python3
"""Streaming rate of the coefficient operators (ops_kernels.hpp) on a 4096^2 db4 L4 plan and a 2048^2 haar L5 SWT plan:
pipelined microseconds per call and GB/s of the bytes the operator must move (read + write of the coefficients it touches)."""
import sys
import time
sys.path.insert(0, '.')
import numpy as np
from pypwt_amd import Wavelets


def t(fn, sync, n=50):
    for _ in range(5):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return (time.perf_counter() - t0) / n * 1e6


for shape, wname, L, swt in (((4096, 4096), "db4", 4, 0), ((2048, 2048), "haar", 5, 1), ((1, 1 << 24), "sym8", 6, 0)):
    x = (np.random.RandomState(1).rand(*shape) * 255).astype(np.float32)
    W = Wavelets(x if shape[0] > 1 else x[0], wname, L, do_swt=swt, ndim=2 if shape[0] > 1 else 1)
    W2 = Wavelets(x if shape[0] > 1 else x[0], wname, L, do_swt=swt, ndim=2 if shape[0] > 1 else 1)
    W.forward(); W2.forward()
    n = shape[0] * shape[1]
    ncoef = n * ((3 * L + 1) if (swt and shape[0] > 1) else 1)
    ndet = ncoef - (n if swt else n // (4 ** L if shape[0] > 1 else 2 ** L))
    print("# %s %s L%d%s: %d coefficients" % ("x".join(map(str, shape)), wname, L, " swt" if swt else "", ncoef))
    for name, fn, nbytes in (
        ("hard_threshold", lambda: W.hard_threshold(1.0), 8 * ndet),
        ("soft_threshold(app)", lambda: (W.soft_threshold(1.0, 1), W.norm1()), 8 * ncoef + 4 * ncoef),
        ("shrink", lambda: W.shrink(0.5), 8 * ncoef),
        ("proj_linf", lambda: W.proj_linf(100.0), 8 * ncoef),
        ("soft_threshold+norm1", lambda: (W.soft_threshold(1.0), W.norm1()), 8 * ndet + 4 * ncoef),
        ("soft_threshold_norms", lambda: W.soft_threshold_norms(1.0), 8 * ndet + 4 * (ncoef - ndet)),   # one sweep, results stay on the device
        ("norms_device", W.norms_device, 4 * ncoef),   # no round trip
        ("norm1", W.norm1, 4 * ncoef),
        ("norm2sq", W.norm2sq, 4 * ncoef),
        ("add_wavelet", lambda: W.add_wavelet(W2, 0.5), 12 * ncoef),
    ):
        us = t(fn, W.synchronize)
        print("  %-22s %8.1f us  %7.0f GB/s" % (name, us, nbytes / us / 1e3))


# ---------------------------------------------------------------------------------------------------------------------
# The per (band, image) operators (band_stats, estimate_sigma, threshold_bands, denoise; select_magnitude, keep_largest) next to the whole-arena sweeps that
# move the same bytes, on the default config's plans (4096^2 db4 L4, batch 1 and 16) and the SWT config's (2048^2 haar L5).
# Hash input: the detail bands are noise-like, which is what the first pass of the select has to cope with.
from collections import defaultdict

from pypwt_amd import BatchedWavelets

for batch, N, wname, L, swt in ((1, 4096, "db4", 4, 0), (16, 4096, "db4", 4, 0), (1, 2048, "haar", 5, 1)):
    B = BatchedWavelets(batch, N, N, wname, L, do_swt=swt)
    B.fill_hash(1, 255.0)
    B.forward()
    n = batch * N * N
    ncoef = n * ((3 * L + 1) if swt else 1)
    ndet = ncoef - (n if swt else n // 4 ** L)
    nnoise = n if swt else n // 4
    print("# adaptive: %d x %d^2 %s L%d%s: %d coefficients, noise band %d" % (batch, N, wname, L, " swt" if swt else "", ncoef, nnoise))
    table = np.full((B.nbands, batch), 1e-3, dtype=np.float32)
    table[0] = np.nan
    B.threshold_bands(table)                                        # host table once: it now sits in the plan's slot ...
    dtab = B._adaptive_view(B._adaptive_slots()[2], table.shape, np.float32)   # ... and is read from there (no upload per call)
    for name, fn, nbytes in (
        ("hard_threshold", lambda: B._lib.pdwt_hard_threshold(B._h, 1e-3, 0, 0), 8 * ndet),
        ("threshold_bands", lambda: B.threshold_bands(dtab), 8 * ndet),
        ("threshold_bands(hard)", lambda: B.threshold_bands(dtab, "hard"), 8 * ndet),
        ("norms_device", B.norms_device, 4 * ncoef),
        ("band_stats", B.band_stats, 4 * ncoef),
        ("estimate_sigma", B.estimate_sigma, 4 * nnoise * 3),
        ("denoise(BayesShrink)", B.denoise, 4 * nnoise * 3 + 4 * ncoef + 8 * ndet),
        ("denoise(sigma given)", lambda: B.denoise(sigma=1.0), 4 * ncoef + 8 * ndet),
        ("fwd+soft+inv (parent)", lambda: (B.forward(), B.soft_threshold(1.0), B.inverse()), 0),
        ("fwd+denoise+inv", lambda: (B.forward(), B.denoise(), B.inverse()), 0),
    ):
        B.forward()
        us = t(fn, B.synchronize, 30)
        print("  %-22s %8.1f us" % (name, us) + ("  %7.0f GB/s" % (nbytes / us / 1e3) if nbytes else ""))
    # the select pass by pass (per-launch event timing: a few us of overhead per launch)
    B.forward()
    B.enable_kernel_timing(True)
    B.reset_kernel_times()
    for _ in range(20):
        B.estimate_sigma()
    B.synchronize()
    acc = defaultdict(list)
    for name, ms in B.kernel_times():
        acc[name].append(ms * 1e3)
    for name in sorted(acc):
        us = float(np.median(acc[name]))
        rate = "  %7.0f GB/s read" % (4 * nnoise / us / 1e3) if name.startswith("select_hist") else ""
        print("  %-22s %8.1f us%s" % (name, us, rate))
    B.enable_kernel_timing(False)

    # ---- best K-term approximation (select_magnitude, keep_largest) next to the parent operators with the same inner loops, in
    # the SAME run: every row three times (median, min-max: the run-to-run spread a difference has to exceed).  K = 10 % of the
    # detail coefficients.  keep_largest zeroes 90 % of them, so "keep_largest (repeated)" selects on sparse data from the second
    # call on (most elements in ONE first-pass bin); "forward + ..." feeds fresh coefficients every call.
    def t3(fn):
        r = sorted(t(fn, B.synchronize, 30) for _ in range(3))
        return r[1], r[0], r[2]

    print("# sparsify: K = N / 10, N = %d detail coefficients per image" % (ndet // batch))
    for name, fn, nbytes in (
        ("hard_threshold", lambda: B._lib.pdwt_hard_threshold(B._h, 1e-3, 0, 0), 8 * ndet),
        ("estimate_sigma", B.estimate_sigma, 4 * nnoise * 3),
        ("select_magnitude", lambda: B.select_magnitude(fraction=0.1), 4 * ndet * 3),
        ("forward", B.forward, 0),
        ("forward+hard_threshold", lambda: (B.forward(), B._lib.pdwt_hard_threshold(B._h, 1e-3, 0, 0)), 0),
        ("forward+keep_largest", lambda: (B.forward(), B.keep_largest(fraction=0.1)), 0),
        ("keep_largest (repeated)", lambda: B.keep_largest(fraction=0.1), 4 * ndet * 3 + 8 * ndet),
    ):
        B.forward()
        us, lo, hi = t3(fn)
        print("  %-24s %8.1f us  (%.1f - %.1f)" % (name, us, lo, hi) + ("  %7.0f GB/s" % (nbytes / us / 1e3) if nbytes else ""))
    # pass by pass, event-timed, on fresh coefficients: the select over all detail bands next to the one over the noise band,
    # the keep sweep next to the parent's hard_threshold sweep
    B.enable_kernel_timing(True)
    B.reset_kernel_times()
    for _ in range(20):
        B.forward()
        B.estimate_sigma()
        B._lib.pdwt_hard_threshold(B._h, 1e-3, 0, 0)
        B.forward()
        B.keep_largest(fraction=0.1)
    B.synchronize()
    acc = defaultdict(list)
    for name, ms in B.kernel_times():
        acc[name].append(ms * 1e3)
    for name in sorted(acc):
        if not (name.startswith("select_") or name in ("keep_bands", "hard_threshold")):
            continue
        v = np.sort(np.array(acc[name]))
        us = float(np.median(v))
        nbytes = 4 * ndet if name.startswith("select_hist_bands") else 4 * nnoise if name.startswith("select_hist") else \
            8 * ndet if name in ("keep_bands", "hard_threshold") else 0
        rate = "  %7.0f GB/s" % (nbytes / us / 1e3) if nbytes else ""
        print("  %-24s %8.1f us  (%.1f - %.1f, quartiles)%s" % (name, us, v[len(v) // 4], v[(3 * len(v)) // 4], rate))
    B.enable_kernel_timing(False)
    del B
