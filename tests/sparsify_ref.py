"""Plain numpy restatement of the best K-term approximation (select_magnitude, keep_largest).

Bands come as in adaptive_ref: the plan's order (band 0 = approximation), every band a (batch, rows, cols) array.  Per image:

  S        the swept bands: the detail bands, and band 0 with `do_app`; N = their elements
  key(c)   the bit pattern of |c| as an unsigned integer: orders like |c|, NaNs behind +inf, -0.0 == +0.0 == 0
  K        clamped to [0, N];  K == 0: everything becomes +0.0, threshold +inf, kept 0;  K >= N: nothing changes, threshold 0,
           kept N;  else t = np.sort(keys)[N - K] (the K-th largest), kept = #(key >= key(t)) (ties at t all survive, so
           kept >= K), and c stays bit for bit iff key(c) >= key(t), else it becomes +0.0

tests/test_sparsify_ref_cpu.py pins this to np.partition on tie-free data and to hand-written tie, NaN and inf cases.
"""
import numpy as np


def key_dtype(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def keys(x):
    """The bit pattern of |x|."""
    x = np.ascontiguousarray(x)
    u = x.view(key_dtype(x.dtype))
    return u & (~u.dtype.type(0) >> u.dtype.type(1))


def value(key, dtype):
    return np.array([key], dtype=key_dtype(dtype)).view(dtype)[0]


def select_key(all_keys, k):
    """(key of the threshold or None when nothing is kept, threshold as a value, kept) of one image's keys (1D)."""
    n = all_keys.size
    dt = np.float32 if all_keys.dtype == np.uint32 else np.float64
    k = min(max(int(k), 0), n)
    if k == 0:
        return None, dt(np.inf), 0
    if k >= n:
        return all_keys.dtype.type(0), dt(0), n
    t = np.sort(all_keys)[n - k]
    return t, value(t, dt), int(np.count_nonzero(all_keys >= t))


def swept(bands, do_app=0):
    return range(0 if do_app else 1, len(bands))


def count(bands, do_app=0):
    """N: elements per image of the swept bands."""
    return sum(bands[b][0].size for b in swept(bands, do_app))


def per_image(k, batch):
    k = np.asarray(k, dtype=np.int64).reshape(-1)
    return np.broadcast_to(k, (batch,)) if k.size == 1 else k


def select_magnitude(bands, k, do_app=0):
    """(threshold[batch] in the bands' type, kept[batch] uint64)."""
    batch = bands[0].shape[0]
    ks = per_image(k, batch)
    thr = np.zeros(batch, dtype=bands[0].dtype)
    kept = np.zeros(batch, dtype=np.uint64)
    for i in range(batch):
        allk = np.concatenate([keys(bands[b][i]).ravel() for b in swept(bands, do_app)])
        _, thr[i], kept[i] = select_key(allk, ks[i])
    return thr, kept


def keep_largest(bands, k, do_app=0):
    """(threshold[batch], kept[batch], the bands after the sweep)."""
    batch = bands[0].shape[0]
    ks = per_image(k, batch)
    thr = np.zeros(batch, dtype=bands[0].dtype)
    kept = np.zeros(batch, dtype=np.uint64)
    out = [b.copy() for b in bands]
    for i in range(batch):
        allk = np.concatenate([keys(bands[b][i]).ravel() for b in swept(bands, do_app)])
        t, thr[i], kept[i] = select_key(allk, ks[i])
        for b in swept(bands, do_app):
            if t is None:
                out[b][i] = 0
            else:
                out[b][i] = np.where(keys(bands[b][i]) >= t, bands[b][i], bands[b].dtype.type(0))
    return thr, kept, out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(key_dtype(a.dtype)), b.view(key_dtype(b.dtype)))
