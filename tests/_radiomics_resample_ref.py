"""The numpy restatement of `mmnn_normalize_scan` and `mmnn_resample_pair` (include/mmnn_sts.h), in the contracts' own order, and the
independent check of the resampling against scipy.

    normalize_stats(scan, scale)                       (n, mean, sd): two passes, divisor n - 1, fp64 (numpy's own summation order)
    normalize(scan, scan_scale, scale, outliers, mean, sd)   the normalised volume, float32; mean / sd None: those of normalize_stats
    prefilter(v, K)                                    the cubic B-spline coefficients of an fp64 volume, along x, then y, then z
    evaluate(coef, shape, tables)                      the three separable 4-tap gathers, fp64
    restate(scan, mask, grid, tables, K, ...)          (float32 scan, uint8 mask) on the new grid
    coordinates(grid)                                  c_a(j) per axis;  by_scipy(v, grid): spline_filter + map_coordinates

Arrays are indexed [x, y, z] as everywhere in these tests (the device holds them x fastest).  The recursions are vectorised across
lines with a Python loop along the line; every sum is `acc = acc + w * v` from a zero array, one product and one addition per term, the
order the kernels keep per output, so the comparison on the device is bitwise."""
import numpy as np

from tests._radiomics_log_ref import scaled

TOL = 2.0 ** -40


def normalize_stats(scan, scan_scale=(1.0, 0.0)):
    v = scaled(scan, scan_scale)
    n = v.size
    with np.errstate(all="ignore"):
        mean = v.sum() / n
        sd = np.sqrt(((v - mean) ** 2).sum() / np.float64(n - 1))
    return n, float(mean), float(sd)


def normalize(scan, scan_scale=(1.0, 0.0), scale=100.0, outliers=0.0, mean=None, sd=None):
    v = scaled(scan, scan_scale)
    if mean is None:
        _, mean, sd = normalize_stats(scan, scan_scale)
    with np.errstate(all="ignore"):
        u = ((v - np.float64(mean)) / np.float64(sd)) * np.float64(scale)
        if outliers > 0.0:
            b = np.float64(outliers) * np.float64(scale)
            u = np.where(u < -b, -b, np.where(u > b, b, u))           # a NaN fails both comparisons and stays
        return u.astype(np.float32)


def mirror(k, n):
    """Whole-sample symmetric reflection into 0 .. n - 1, period 2 n - 2; 0 for n = 1."""
    if n == 1:
        return 0
    r = k % (2 * n - 2)
    return r if r < n else 2 * n - 2 - r


def prefilter_axis(v, axis, K):
    n = v.shape[axis]
    if n == 1:
        return v
    z, zp = np.float64(K["pole"]), K["pole_power"]
    with np.errstate(all="ignore"):
        s = np.float64(K["gain"]) * np.moveaxis(v, axis, 0)
        cp = np.empty_like(s)
        acc = np.zeros(s.shape[1:])
        for k in range(len(zp)):
            acc = acc + zp[k] * s[mirror(k, n)]
        cp[0] = acc
        for k in range(1, n):
            cp[k] = s[k] + z * cp[k - 1]
        cm = np.empty_like(s)
        cm[n - 1] = np.float64(K["pole_gain"]) * (cp[n - 1] + z * cp[n - 2])
        for k in range(n - 2, -1, -1):
            cm[k] = z * (cm[k + 1] - cp[k])
    return np.moveaxis(cm, 0, axis)


def prefilter(v, K):
    for axis in range(3):
        v = prefilter_axis(v, axis, K)
    return v


def split_tables(out_shape, tables):
    mx, my, mz = out_shape
    assert len(tables) == mx + my + mz
    return tables[:mx], tables[mx:mx + my], tables[mx + my:]


def gather(v, e, axis):
    shape = [1, 1, 1]
    shape[axis] = len(e)
    out = np.zeros(v.shape[:axis] + (len(e),) + v.shape[axis + 1:])
    with np.errstate(all="ignore"):
        for k in range(4):
            out = out + e["w"][:, k].reshape(shape) * np.take(v, e["i"][:, k], axis=axis)
    return out


def evaluate(coef, out_shape, tables):
    for axis, e in enumerate(split_tables(out_shape, tables)):
        coef = gather(coef, e, axis)
    return coef


def inside_of(out_shape, tables):
    ex, ey, ez = split_tables(out_shape, tables)
    return (ex["inside"] != 0)[:, None, None] & (ey["inside"] != 0)[None, :, None] & (ez["inside"] != 0)[None, None, :]


def restate(scan, mask, grid, tables, K, scan_scale=(1.0, 0.0), mask_scale=(1.0, 0.0)):
    ex, ey, ez = split_tables(grid.shape, tables)
    inside = inside_of(grid.shape, tables)
    with np.errstate(all="ignore"):
        val = evaluate(prefilter(scaled(scan, scan_scale), K), grid.shape, tables).astype(np.float32)
    near = scaled(mask, mask_scale)[np.ix_(ex["nearest"], ey["nearest"], ez["nearest"])]
    return np.where(inside, val, np.float32(0.0)), (inside & ~(near == 0.0)).astype(np.uint8)


def coordinates(grid):
    """c_a(j) = (j + 0.5) r_a - 0.5 per axis."""
    return [(np.arange(m, dtype=np.float64) + 0.5) * float(r) - 0.5 for m, r in zip(grid.shape, grid.ratio)]


def by_scipy(v, grid):
    """(coefficients, values at c(j)) from scipy.ndimage: an implementation that shares nothing with the restatement."""
    from scipy import ndimage
    coef = ndimage.spline_filter(v, order=3, mode="mirror", output=np.float64)
    pts = np.meshgrid(*coordinates(grid), indexing="ij")
    return coef, ndimage.map_coordinates(v, pts, order=3, mode="mirror", output=np.float64)
