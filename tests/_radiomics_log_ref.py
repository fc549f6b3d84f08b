"""The numpy restatement of `mmnn_log_filter` (include/mmnn_sts.h), in the contract's own order, and its independent check against scipy.

    restate(scan, radius, taps, weight, scale)   the filtered volume, float32 (x, y, z); fp64 with `rounded=False`
    by_scipy(v, sigma_mm, spacing)               the same image from scipy.ndimage.gaussian_filter, fp64
    scale_S(v, taps, radius, weight)             S = max|v| sum_a w_a ||h_a||_1, the scale both tolerances are relative to

Arrays are indexed [x, y, z] as everywhere in these tests (the device holds them x fastest).  Every sum is literally
`out += w[t] * take(v, clip(i + t))` for t = -r .. +r from a zero array: one product and one addition per tap, fp64, the order the kernel
keeps per output, so the comparison on the device is bitwise."""
import numpy as np

TOL = 2.0 ** -40


def scaled(scan, scale=(1.0, 0.0)):
    """raw * slope + inter in fp64, two roundings; a slope of 0 (or the pair 1, 0) leaves the raw value."""
    v = np.asarray(scan).astype(np.float64)
    slope, inter = float(scale[0]), float(scale[1])
    if slope == 0.0 or not np.isfinite(slope) or (slope == 1.0 and inter == 0.0):
        return v
    return v * slope + inter


def fir(v, w, axis):
    r = (len(w) - 1) // 2
    n = v.shape[axis]
    idx = np.arange(n)
    out = np.zeros_like(v)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(-r, r + 1):
            out += w[t + r] * np.take(v, np.clip(idx + t, 0, n - 1), axis=axis)
    return out


def split_taps(radius, taps):
    """taps -> [(g_x, h_x), (g_y, h_y), (g_z, h_z)]."""
    out, o = [], 0
    for r in radius:
        n = 2 * int(r) + 1
        out.append((taps[o:o + n], taps[o + n:o + 2 * n]))
        o += 2 * n
    assert o == len(taps)
    return out


def restate(scan, radius, taps, weight, scale=(1.0, 0.0), rounded=True):
    (gx, hx), (gy, hy), (gz, hz) = split_taps(radius, taps)
    v = scaled(scan, scale)
    a0, a2 = fir(v, gx, 0), fir(v, hx, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        b0 = fir(a0, gy, 1)
        c = fir(a2, gy, 1) * weight[0] + fir(a0, hy, 1) * weight[1]
        out = fir(c, gz, 2) + fir(b0, hz, 2) * weight[2]
        return out.astype(np.float32) if rounded else out


def scale_S(v, radius, taps, weight):
    return float(np.abs(v).max()) * sum(float(w) * float(np.abs(h).sum()) for (_, h), w in zip(split_taps(radius, taps), weight))


def by_scipy(v, sigma_mm, spacing):
    """sum_a w_a (G with order 2 along a - d_a.sum() G with order 0): scipy's sampled derivative kernel is d, the contract's is
    h = d - g d.sum()."""
    from scipy import ndimage
    sv = [float(sigma_mm) / float(s) for s in spacing]
    smooth = ndimage.gaussian_filter(v, sv, order=0, mode="nearest", truncate=4.0)
    out = np.zeros_like(v)
    for a in range(3):
        r = int(4.0 * sv[a] + 0.5)
        k = np.arange(-r, r + 1, dtype=np.float64)
        g = np.exp(-(k * k) / (2.0 * sv[a] * sv[a]))
        g /= g.sum()
        d = ((k * k) / sv[a] ** 4 - 1.0 / (sv[a] * sv[a])) * g
        order = [0, 0, 0]
        order[a] = 2
        out += (float(sigma_mm) / float(spacing[a])) ** 2 * (ndimage.gaussian_filter(v, sv, order=order, mode="nearest", truncate=4.0) - d.sum() * smooth)
    return out
