"""Plain numpy reference of the proximal operators of a volume (`Wavelets3D.group_soft_threshold`, `group_norm`, `proj_linf`,
`shrink`, `add_wavelet`), for decimated and stationary volumes alike: they work on the sub-bands in `num` order (tests/volume_ref.py:
0 = A_L, then 1 + 7 (l - 1) + k over 'aad' .. 'ddd'), whatever their shapes.

  * `group_soft` is tests/ops_ref.py's arithmetic -- float64 for float32 bands, np.longdouble for float64 bands, rounded once at
    the end -- with groups of `per` detail sub-bands per level (7 for a volume) and A_L in the group of the last level when
    `do_app`;
  * `group_norm` is the l2,1 norm of the same groups in np.longdouble;
  * `linf`, `shrink` and `axpy` are ops_ref's, band by band.
tests/test_volume_prox_ref_cpu.py pins these to things that are not them.
"""
import numpy as np

import ops_ref

PER = 7


def groups(levels, do_app=0, per=PER):
    """[[num, ...]] of level 1 .. levels: the members of that level's groups."""
    out = []
    for l in range(1, levels + 1):
        idx = [per * (l - 1) + 1 + k for k in range(per)]
        if do_app and l == levels:
            idx.append(0)
        out.append(idx)
    return out


def group_soft(bands, levels, beta, do_app=0, normalize=0, per=PER):
    """Every member of a group times max(1 - beta_l / ||g||_2, 0), 0 where the norm is 0; beta_l = ops_ref.level_betas."""
    dt = bands[0].dtype.type
    wide = np.float64 if dt is np.float32 else np.longdouble
    assert len(bands) == per * levels + 1
    betas = ops_ref.level_betas(beta, levels, normalize, dt)
    out = [b.copy() for b in bands]
    for l, idx in enumerate(groups(levels, do_app, per), 1):
        grp = [bands[i].astype(wide) for i in idx]
        nrm = np.sqrt(sum(g * g for g in grp))
        with np.errstate(divide="ignore", invalid="ignore"):
            res = np.where(nrm == 0, wide(0), np.fmax(wide(1) - wide(betas[l - 1]) / nrm, wide(0)))
        for i, g in zip(idx, grp):
            out[i] = (g * res).astype(dt)
    return out


def zeroed_fraction(bands, levels, beta, do_app=0, normalize=0, per=PER):
    """The share of the groups whose norm is at most their beta_l (they become zero)."""
    dt = bands[0].dtype.type
    betas = ops_ref.level_betas(beta, levels, normalize, dt)
    zero = total = 0
    for l, idx in enumerate(groups(levels, do_app, per), 1):
        nrm = np.sqrt(sum(bands[i].astype(np.longdouble) ** 2 for i in idx))
        zero += int(np.count_nonzero(nrm <= np.longdouble(betas[l - 1])))
        total += nrm.size
    return zero / total


def group_norm(bands, levels, do_app=0, per=PER):
    """sum over levels and positions of ||g||_2, in np.longdouble."""
    s = np.longdouble(0)
    for idx in groups(levels, do_app, per):
        s += np.sqrt(sum(bands[i].astype(np.longdouble) ** 2 for i in idx)).sum(dtype=np.longdouble)
    return s


def linf(bands, beta, do_app=1):
    return [ops_ref.linf(bands[0], beta) if do_app else bands[0].copy()] + [ops_ref.linf(b, beta) for b in bands[1:]]


def shrink(bands, beta, do_app=1):
    return ops_ref.shrink(bands, beta, do_app)


def axpy(dst, src, alpha):
    return ops_ref.axpy(dst, src, alpha)
