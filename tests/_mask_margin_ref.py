"""The rule of `mmnn_mask_margin` (include/mmnn_sts.h) restated in numpy fp64, host only.  Arrays are (x, y, z), as a NIfTI reader returns
them.

    set_voxels(raw, slope, inter)          the set voxels: !(m == 0), m = raw * slope + inter in fp64 (two roundings), a NaN is set
    term(k, s)                             t_a(k) = fl(fl(k s) fl(k s))
    reach(spacing, radius)                 per axis the largest k with t_a(k) <= fl(radius radius)
    brute(flags, spacing)                  D(p) = min over set q of fl(fl(t_x + t_y) + t_z): a loop over all set voxels
    separable(flags, spacing, reach=None)  the same D by three passes x, y, z; with `reach` every pass looks no farther than that, and D is
                                           then only meant where it is <= R2
    threshold(D, radius, mode)             -> (out uint8, dist2): 'dilate' D <= R2, 'shell' 0 < D <= R2; dist2 = D where D <= R2, else +inf
    margin(raw, spacing, radius, mode, slope, inter, how)   all of it

numpy rounds every elementwise operation on its own (no FMA), which is what the rule asks for.
"""
import numpy as np


def set_voxels(raw, slope=1.0, inter=0.0):
    m = np.asarray(raw).astype(np.float64)
    slope, inter = float(slope), float(inter)
    if slope != 0.0 and np.isfinite(slope):
        inter = inter if np.isfinite(inter) else 0.0
        if not (slope == 1.0 and inter == 0.0):
            m = m * slope + inter
    return ~(m == 0.0)


def term(k, s):
    d = np.asarray(k, dtype=np.float64) * np.float64(s)
    return d * d


def reach(spacing, radius):
    r2 = np.float64(radius) * np.float64(radius)
    out = []
    for s in spacing:
        k = 0
        while term(k + 1, s) <= r2:
            k += 1
        out.append(k)
    return tuple(out)


def brute(flags, spacing):
    X, Y, Z = flags.shape
    D = np.full(flags.shape, np.inf)
    ix, iy, iz = np.arange(X), np.arange(Y), np.arange(Z)
    for qx, qy, qz in np.argwhere(flags):
        tx, ty, tz = term(np.abs(ix - qx), spacing[0]), term(np.abs(iy - qy), spacing[1]), term(np.abs(iz - qz), spacing[2])
        D = np.minimum(D, (tx[:, None, None] + ty[None, :, None]) + tz[None, None, :])
    return D


def _min_along(A, axis, s, r):
    """min over d = -r .. r of fl(A shifted by d along `axis` + t(|d|)); outside the volume is +inf."""
    n = A.shape[axis]
    B = np.full(A.shape, np.inf)
    for d in range(-r, r + 1):
        t = term(abs(d), s)
        dst = [slice(None)] * 3
        src = [slice(None)] * 3
        dst[axis] = slice(max(0, -d), n - max(0, d))       # p
        src[axis] = slice(max(0, d), n - max(0, -d))       # p + d
        dst, src = tuple(dst), tuple(src)
        B[dst] = np.minimum(B[dst], A[src] + t)
    return B


def separable(flags, spacing, reach=None):
    X, Y, Z = flags.shape
    r = [n - 1 for n in flags.shape] if reach is None else [min(int(k), n - 1) for k, n in zip(reach, flags.shape)]
    ix = np.arange(X)[:, None, None]
    last = np.maximum.accumulate(np.where(flags, ix, -4 * X), axis=0)                     # the nearest set x' <= x
    nxt = np.minimum.accumulate(np.where(flags, ix, 4 * X)[::-1], axis=0)[::-1]          # the nearest set x' >= x
    k = np.minimum(ix - last, nxt - ix)
    A = np.where(k <= r[0], term(np.minimum(k, X), spacing[0]), np.inf)
    return _min_along(_min_along(A, 1, spacing[1], r[1]), 2, spacing[2], r[2])


def threshold(D, radius, mode="dilate"):
    r2 = np.float64(radius) * np.float64(radius)
    inside = D <= r2
    out = inside & (D > 0.0) if mode == "shell" else inside
    return out.astype(np.uint8), np.where(inside, D, np.inf)


def margin(raw, spacing, radius, mode="dilate", slope=1.0, inter=0.0, how="separable"):
    flags = set_voxels(raw, slope, inter)
    D = brute(flags, spacing) if how == "brute" else separable(flags, spacing, reach(spacing, radius))
    return threshold(D, radius, mode)


def random_mask(shape, fraction, seed):
    return (np.random.default_rng(seed).random(shape) < fraction).astype(np.uint8)
