"""numpy fp64 restatement of `mmnn_radiomics` (include/mmnn_sts.h) and of `mmnn_sts_amd.radiomics.finish`, written from the feature
definitions, plus an mpmath evaluation of the same features from the same exact integer counts and values.

Volumes are (x, y, z) arrays, as `nifti.read` returns them.  `restate` returns the integers (n, box, moments, Ng, hist, glcm, order
statistics) and, for every fp64 feature, a pair (value, scale).  The scale is what a rounding error of the evaluation is relative to:
the sum of the absolute values of the terms of the feature's sum (divided by what the sum is divided by), plus, where the terms are
formed from an already rounded centre, the first-order effect of that centre's own error:

    the mean m of the ROI carries an error relative to A = sum|v| / n, and d/dm of sum (v - m)^k / n is -k m_{k-1}: the third and
    fourth central moments and the absolute deviations get k * |m_{k-1}|-like * A added (the second moment is stationary in m);
    the GLCM mean mu is a sum of positive terms, error relative to mu itself: ClusterShade gets 6 * ClusterTendency * mu,
    ClusterProminence 8 * sum|c|^3 p * mu (ClusterTendency, SumSquares, DifferenceVariance are stationary in their centre);
    quotients take the scale of the numerator over the denominator, plus |value| for a denominator that is itself a rounded sum;
    Imc2 = f(x) = sqrt(1 - exp(-2x)), x = HXY2 - HXY, has f' = exp(-2x) / f, so its scale is f + (|HXY2| + |HXY|) exp(-2x) / f, and
    sqrt(2 (|HXY2| + |HXY|)) where f = 0.

A feature averaged over the GLCM directions takes the average of the directions' scales.
"""
import math

import numpy as np

EPS = 2.0 ** -52
PCT = (10.0, 25.0, 50.0, 75.0, 90.0)
DIRECTIONS = [(dz, dy, dx) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
              if (dz, dy, dx) > (0, 0, 0) and next(c for c in (dz, dy, dx) if c != 0) > 0]
FIRSTORDER = ("Energy", "Minimum", "Maximum", "Range", "Mean", "Variance", "Skewness", "Kurtosis", "MeanAbsoluteDeviation",
              "RootMeanSquared", "10Percentile", "90Percentile", "Median", "InterquartileRange", "RobustMeanAbsoluteDeviation", "Entropy",
              "Uniformity")
BITWISE = ("Minimum", "Maximum", "Range", "10Percentile", "90Percentile", "Median", "InterquartileRange")
GLCM = ("Autocorrelation", "JointAverage", "ClusterProminence", "ClusterShade", "ClusterTendency", "Contrast", "Correlation",
        "DifferenceAverage", "DifferenceEntropy", "DifferenceVariance", "JointEnergy", "JointEntropy", "Imc1", "Imc2", "Idm", "Idmn", "Id",
        "Idn", "InverseVariance", "MaximumProbability", "SumAverage", "SumEntropy", "SumSquares")
assert len(DIRECTIONS) == 13 and DIRECTIONS[0] == (0, 0, 1) and DIRECTIONS[1] == (0, 1, -1) and DIRECTIONS[-1] == (1, 1, 1)


def scaled(raw, slope=1.0, inter=0.0):
    """raw * slope + inter in fp64, two roundings; a slope of 0 or a non-finite slope switches the scaling off."""
    v = np.asarray(raw).astype(np.float64)
    if slope == 0.0 or not math.isfinite(slope):
        return v
    inter = inter if math.isfinite(inter) else 0.0
    if slope == 1.0 and inter == 0.0:
        return v
    return v * np.float64(slope) + np.float64(inter)


def glcm_features(G):
    """One direction: (Ng, Ng) integer counts -> {name: (value, scale)}, or None for an empty matrix."""
    S = float(G.sum())
    if S == 0.0:
        return None
    ng = G.shape[0]
    p = G.astype(np.float64) / S
    i = np.arange(1, ng + 1, dtype=np.float64)[:, None]
    j = np.arange(1, ng + 1, dtype=np.float64)[None, :]
    px = p.sum(axis=1)
    mu = float((i[:, 0] * px).sum())
    var = float((((i[:, 0] - mu) ** 2) * px).sum())
    ks = np.arange(2, 2 * ng + 1)
    pp = np.bincount(np.add.outer(np.arange(ng), np.arange(ng)).ravel(), p.ravel(), 2 * ng - 1)
    kd = np.arange(0, ng, dtype=np.float64)
    pm = np.bincount(np.abs(np.subtract.outer(np.arange(ng), np.arange(ng))).ravel(), p.ravel(), ng)
    ks = ks.astype(np.float64)
    pxy = px[:, None] * px[None, :]
    HX = -float((px * np.log2(px + EPS)).sum())
    HXY = -float((p * np.log2(p + EPS)).sum())
    HXY1 = -float((p * np.log2(pxy + EPS)).sum())
    HXY2 = -float((pxy * np.log2(pxy + EPS)).sum())
    aHXY, aHXY1, aHXY2 = (float(np.abs(t).sum()) for t in (p * np.log2(p + EPS), p * np.log2(pxy + EPS), pxy * np.log2(pxy + EPS)))
    aHX = float(np.abs(px * np.log2(px + EPS)).sum())
    c = i + j - 2.0 * mu
    auto = float((p * i * j).sum())
    ct = float((c ** 2 * p).sum())
    c3 = float((np.abs(c) ** 3 * p).sum())
    out = {}
    out["Autocorrelation"] = (auto, auto)
    out["JointAverage"] = (mu, mu)
    out["ClusterProminence"] = (float((c ** 4 * p).sum()), float((c ** 4 * p).sum()) + 8.0 * c3 * mu)
    out["ClusterShade"] = (float((c ** 3 * p).sum()), c3 + 6.0 * ct * mu)
    out["ClusterTendency"] = (ct, ct)
    con = float(((i - j) ** 2 * p).sum())
    out["Contrast"] = (con, con)
    out["Correlation"] = ((auto - mu * mu) / var, (auto + mu * mu) / var + abs((auto - mu * mu) / var)) if var != 0.0 else (1.0, 1.0)
    da = float((kd * pm).sum())
    out["DifferenceAverage"] = (da, da)
    out["DifferenceEntropy"] = (-float((pm * np.log2(pm + EPS)).sum()), float(np.abs(pm * np.log2(pm + EPS)).sum()))
    dv = float(((kd - da) ** 2 * pm).sum())
    out["DifferenceVariance"] = (dv, dv)
    je = float((p * p).sum())
    out["JointEnergy"] = (je, je)
    out["JointEntropy"] = (HXY, aHXY)
    imc1 = (HXY - HXY1) / HX if HX != 0.0 else 0.0
    out["Imc1"] = (imc1, ((aHXY + aHXY1) / aHX + abs(imc1)) if HX != 0.0 else 1.0)
    if HXY > HXY2:
        out["Imc2"] = (0.0, math.sqrt(2.0 * (aHXY2 + aHXY)))
    else:
        x = HXY2 - HXY
        f = math.sqrt(1.0 - math.exp(-2.0 * x))
        out["Imc2"] = (f, f + (aHXY2 + aHXY) * math.exp(-2.0 * x) / f) if f > 0.0 else (0.0, math.sqrt(2.0 * (aHXY2 + aHXY)))
    for name, t in (("Idm", pm / (1.0 + kd * kd)), ("Idmn", pm / (1.0 + kd * kd / float(ng * ng))), ("Id", pm / (1.0 + kd)),
                    ("Idn", pm / (1.0 + kd / float(ng))), ("InverseVariance", pm[1:] / (kd[1:] * kd[1:]))):
        out[name] = (float(t.sum()), float(t.sum()))
    out["MaximumProbability"] = (float(p.max()), float(p.max()))
    out["SumAverage"] = (float((ks * pp).sum()), float((ks * pp).sum()))
    out["SumEntropy"] = (-float((pp * np.log2(pp + EPS)).sum()), float(np.abs(pp * np.log2(pp + EPS)).sum()))
    out["SumSquares"] = (var, var)
    return out


def count_glcm(B, ng, max_bins):
    """B: (x, y, z) bins, 0 outside the ROI -> (13, max_bins, max_bins) int64."""
    G = np.zeros((13, max_bins, max_bins), dtype=np.int64)
    X, Y, Z = B.shape
    for d, (dz, dy, dx) in enumerate(DIRECTIONS):
        def cut(n, s):
            return (slice(max(0, -s), n - max(0, s)), slice(max(0, s), n - max(0, -s)))
        (ax, bx), (ay, by), (az, bz) = cut(X, dx), cut(Y, dy), cut(Z, dz)
        a, b = B[ax, ay, az], B[bx, by, bz]
        ok = (a > 0) & (b > 0)
        np.add.at(G[d], (a[ok] - 1, b[ok] - 1), 1)
        np.add.at(G[d], (b[ok] - 1, a[ok] - 1), 1)
    return G


def restate(scan, mask, bin_width=25.0, max_bins=256, scan_scale=(1.0, 0.0), mask_scale=(1.0, 0.0)):
    V = scaled(scan, *scan_scale)
    roi = scaled(mask, *mask_scale) != 0.0
    out = {"hist": np.zeros(max_bins, dtype=np.int64), "glcm": np.zeros((13, max_bins, max_bins), dtype=np.int64)}
    idx = np.argwhere(roi).astype(np.int64)
    n = len(idx)
    out["n"] = n
    out["lo"] = idx.min(axis=0) if n else np.zeros(3, dtype=np.int64)
    out["hi"] = idx.max(axis=0) if n else np.zeros(3, dtype=np.int64)
    x, y, z = (idx[:, k] for k in range(3))
    out["moments"] = np.array([x.sum(), y.sum(), z.sum(), (x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(), (x * z).sum(), (y * z).sum()],
                              dtype=np.int64)
    v = V.T[roi.T]                          # the ROI's values, x fastest
    out["values"] = v
    out["empty"], out["nonfinite"] = n == 0, bool(n and not np.isfinite(v).all())
    out["overflow"], out["n_bins"] = False, 0
    nan = float("nan")
    out["order"] = np.full(10, nan)
    out["firstorder"] = {k: (nan, nan) for k in FIRSTORDER}
    out["glcm_features"] = {k: (nan, nan) for k in GLCM}
    if out["empty"] or out["nonfinite"]:
        return out
    bw = np.float64(bin_width)
    mn, mx = v.min(), v.max()
    low = np.floor(mn / bw) * bw
    bins = np.maximum(np.floor((v - low) / bw) + 1.0, 1.0)
    ng = int(bins.max())
    out["n_bins"] = ng
    if ng > max_bins:
        out["overflow"] = True
        return out
    out["hist"] = np.bincount(bins.astype(np.int64) - 1, minlength=max_bins)
    B = np.zeros(V.shape, dtype=np.int64)
    B.T[roi.T] = bins.astype(np.int64)
    out["bins"] = B
    out["glcm"] = count_glcm(B, ng, max_bins)
    s = np.sort(v)
    order, q = [], []
    for p in PCT:
        h = (n - 1) * p / 100.0
        lo_, hi_ = s[int(math.floor(h))], s[int(math.ceil(h))]
        order += [lo_, hi_]
        q.append(lo_ + (hi_ - lo_) * (h - math.floor(h)))
    out["order"] = np.array(order)
    mean = v.sum() / n
    A = float(np.abs(v).sum() / n)
    d = v - mean
    m2, m3, m4 = (float((d ** k).sum() / n) for k in (2, 3, 4))
    a3 = float((np.abs(d) ** 3).sum() / n)
    mad = float(np.abs(d).sum() / n)
    fo = {}
    en = float((v * v).sum())
    fo["Energy"] = (en, en)
    fo["Minimum"], fo["Maximum"], fo["Range"] = (float(mn), abs(float(mn))), (float(mx), abs(float(mx))), (float(mx - mn), abs(float(mx)) + abs(float(mn)))
    fo["Mean"] = (float(mean), A)
    fo["Variance"] = (m2, m2)
    fo["Skewness"] = (m3 / m2 ** 1.5, (a3 + 3.0 * m2 * A) / m2 ** 1.5) if m2 != 0.0 else (0.0, 1.0)
    fo["Kurtosis"] = (m4 / (m2 * m2), (m4 + 4.0 * a3 * A) / (m2 * m2)) if m2 != 0.0 else (0.0, 1.0)
    fo["MeanAbsoluteDeviation"] = (mad, mad + A)
    fo["RootMeanSquared"] = (math.sqrt(en / n), math.sqrt(en / n))
    fo["10Percentile"], fo["90Percentile"], fo["Median"] = (float(q[0]), abs(float(q[0]))), (float(q[4]), abs(float(q[4]))), (float(q[2]), abs(float(q[2])))
    fo["InterquartileRange"] = (float(q[3] - q[1]), abs(float(q[3])) + abs(float(q[1])))
    inside = v[(v >= q[0]) & (v <= q[4])]
    if len(inside):
        rm = inside.sum() / len(inside)
        fo["RobustMeanAbsoluteDeviation"] = (float(np.abs(inside - rm).sum() / len(inside)),
                                             float(np.abs(inside - rm).sum() / len(inside) + np.abs(inside).sum() / len(inside)))
    else:
        fo["RobustMeanAbsoluteDeviation"] = (nan, nan)
    ph = out["hist"][:ng].astype(np.float64) / n
    fo["Entropy"] = (-float((ph * np.log2(ph + EPS)).sum()), float(np.abs(ph * np.log2(ph + EPS)).sum()))
    fo["Uniformity"] = (float((ph * ph).sum()), float((ph * ph).sum()))
    out["firstorder"] = fo
    per = [f for f in (glcm_features(out["glcm"][d_, :ng, :ng]) for d_ in range(13)) if f is not None]
    if per:
        out["glcm_features"] = {k: (sum(f[k][0] for f in per) / len(per), sum(f[k][1] for f in per) / len(per)) for k in GLCM}
    return out


def shape_reference(roi, linear=None):
    """The six voxel-based shape features straight from the ROI's physical coordinates (np.cov, np.linalg.eigvalsh)."""
    L = np.eye(3) if linear is None else np.asarray(linear, dtype=np.float64)[:3, :3]
    idx = np.argwhere(roi).astype(np.float64)
    pts = idx @ L.T
    cov = np.cov(pts.T, bias=True).reshape(3, 3)
    lam = np.maximum(np.sort(np.linalg.eigvalsh(cov))[::-1], 0.0)
    return {"VoxelVolume": len(idx) * abs(np.linalg.det(L)), "MajorAxisLength": 4 * math.sqrt(lam[0]), "MinorAxisLength": 4 * math.sqrt(lam[1]),
            "LeastAxisLength": 4 * math.sqrt(lam[2]), "Elongation": math.sqrt(lam[1] / lam[0]) if lam[0] > 0 else float("nan"),
            "Flatness": math.sqrt(lam[2] / lam[0]) if lam[0] > 0 else float("nan")}


# ---- the same features in extended precision ---------------------------------------------------------------------------------------
def exact(ref):
    """mpmath (40 digits) evaluation of the moment-based first-order features, Entropy, Uniformity and the 23 GLCM features, from the
    exact inputs of `ref` = restate(...): the ROI's fp64 values, the histogram, the matrices.  Sums whose terms depend on integer
    counts only are grouped by those counts (exact regrouping; it keeps the number of logarithms small)."""
    import mpmath as mp
    mp.mp.dps = 40
    eps, ln2 = mp.mpf(2) ** -52, mp.log(2)

    def lg(x):
        return mp.log(x + eps) / ln2

    v = [mp.mpf(float(t)) for t in ref["values"]]
    n = len(v)
    out = {}
    mean = mp.fsum(v) / n
    d = [t - mean for t in v]
    m2, m3, m4 = (mp.fsum(t ** k for t in d) / n for k in (2, 3, 4))
    en = mp.fsum(t * t for t in v)
    out.update(Energy=en, Mean=mean, Variance=m2, Skewness=(m3 / m2 ** mp.mpf(1.5)) if m2 != 0 else mp.mpf(0),
               Kurtosis=(m4 / (m2 * m2)) if m2 != 0 else mp.mpf(0), MeanAbsoluteDeviation=mp.fsum(abs(t) for t in d) / n,
               RootMeanSquared=mp.sqrt(en / n))
    q10, q90 = float(ref["firstorder"]["10Percentile"][0]), float(ref["firstorder"]["90Percentile"][0])
    inside = [t for t in v if q10 <= t <= q90]
    if inside:
        rm = mp.fsum(inside) / len(inside)
        out["RobustMeanAbsoluteDeviation"] = mp.fsum(abs(t - rm) for t in inside) / len(inside)
    else:
        out["RobustMeanAbsoluteDeviation"] = mp.nan
    ng = ref["n_bins"]
    hist = [int(c) for c in ref["hist"][:ng]]
    out["Entropy"] = -mp.fsum((mp.mpf(c) / n) * lg(mp.mpf(c) / n) for c in hist)
    out["Uniformity"] = mp.fsum((mp.mpf(c) / n) ** 2 for c in hist)
    per = []
    for dct in range(13):
        G = ref["glcm"][dct, :ng, :ng]
        S = int(G.sum())
        if S == 0:
            continue
        Sm = mp.mpf(S)
        row = [int(c) for c in G.sum(axis=1)]
        nz = [(int(i), int(j), int(G[i, j])) for i, j in zip(*np.nonzero(G))]
        plus, minus = {}, {}
        for i, j, c in nz:
            plus[i + j + 2] = plus.get(i + j + 2, 0) + c
            minus[abs(i - j)] = minus.get(abs(i - j), 0) + c
        mu = mp.fsum((i + 1) * mp.mpf(r) / Sm for i, r in enumerate(row))
        var = mp.fsum((i + 1 - mu) ** 2 * mp.mpf(r) / Sm for i, r in enumerate(row))
        HX = -mp.fsum((mp.mpf(r) / Sm) * lg(mp.mpf(r) / Sm) for r in row)
        by_c, by_pair = {}, {}
        for i, j, c in nz:
            by_c[c] = by_c.get(c, 0) + 1
            key = (min(row[i], row[j]), max(row[i], row[j]))
            by_pair[key] = by_pair.get(key, 0) + c
        HXY = -mp.fsum(k * (mp.mpf(c) / Sm) * lg(mp.mpf(c) / Sm) for c, k in by_c.items())
        HXY1 = -mp.fsum((mp.mpf(c) / Sm) * lg(mp.mpf(a) * b / (Sm * Sm)) for (a, b), c in by_pair.items())
        rows = {}
        for r in row:
            if r:
                rows[r] = rows.get(r, 0) + 1
        HXY2 = -mp.fsum(ka * kb * (mp.mpf(a) * b / (Sm * Sm)) * lg(mp.mpf(a) * b / (Sm * Sm)) for a, ka in rows.items() for b, kb in rows.items())
        auto = mp.fsum((i + 1) * (j + 1) * mp.mpf(c) / Sm for i, j, c in nz)
        f = {}
        f["Autocorrelation"], f["JointAverage"] = auto, mu
        for name, k in (("ClusterProminence", 4), ("ClusterShade", 3), ("ClusterTendency", 2)):
            f[name] = mp.fsum((s - 2 * mu) ** k * mp.mpf(c) / Sm for s, c in plus.items())
        f["Contrast"] = mp.fsum(k * k * mp.mpf(c) / Sm for k, c in minus.items())
        f["Correlation"] = (auto - mu * mu) / var if var != 0 else mp.mpf(1)
        da = mp.fsum(k * mp.mpf(c) / Sm for k, c in minus.items())
        f["DifferenceAverage"] = da
        f["DifferenceEntropy"] = -mp.fsum((mp.mpf(c) / Sm) * lg(mp.mpf(c) / Sm) for c in minus.values())
        f["DifferenceVariance"] = mp.fsum((k - da) ** 2 * mp.mpf(c) / Sm for k, c in minus.items())
        f["JointEnergy"] = mp.fsum(k * (mp.mpf(c) / Sm) ** 2 for c, k in by_c.items())
        f["JointEntropy"] = HXY
        f["Imc1"] = (HXY - HXY1) / HX if HX != 0 else mp.mpf(0)
        f["Imc2"] = mp.sqrt(1 - mp.exp(-2 * (HXY2 - HXY))) if HXY2 >= HXY else mp.mpf(0)
        f["Idm"] = mp.fsum(mp.mpf(c) / Sm / (1 + k * k) for k, c in minus.items())
        f["Idmn"] = mp.fsum(mp.mpf(c) / Sm / (1 + mp.mpf(k * k) / (ng * ng)) for k, c in minus.items())
        f["Id"] = mp.fsum(mp.mpf(c) / Sm / (1 + k) for k, c in minus.items())
        f["Idn"] = mp.fsum(mp.mpf(c) / Sm / (1 + mp.mpf(k) / ng) for k, c in minus.items())
        f["InverseVariance"] = mp.fsum(mp.mpf(c) / Sm / (k * k) for k, c in minus.items() if k >= 1)
        f["MaximumProbability"] = mp.mpf(int(G.max())) / Sm
        f["SumAverage"] = mp.fsum(s * mp.mpf(c) / Sm for s, c in plus.items())
        f["SumEntropy"] = -mp.fsum((mp.mpf(c) / Sm) * lg(mp.mpf(c) / Sm) for c in plus.values())
        f["SumSquares"] = var
        per.append(f)
    for k in GLCM:
        out[k] = mp.fsum(f[k] for f in per) / len(per) if per else mp.nan
    return out


TOLERANCED_FIRSTORDER = tuple(k for k in FIRSTORDER if k not in BITWISE)
CLASSES = {"firstorder_moment": ("Energy", "Mean", "Variance", "Skewness", "Kurtosis", "MeanAbsoluteDeviation", "RootMeanSquared",
                                 "RobustMeanAbsoluteDeviation"),
           "histogram": ("Entropy", "Uniformity"),
           "glcm_sum": ("Autocorrelation", "JointAverage", "ClusterProminence", "ClusterShade", "ClusterTendency", "Contrast",
                        "DifferenceAverage", "DifferenceVariance", "JointEnergy", "Idm", "Idmn", "Id", "Idn", "InverseVariance",
                        "MaximumProbability", "SumAverage", "SumSquares", "Correlation"),
           "glcm_entropy": ("DifferenceEntropy", "JointEntropy", "SumEntropy", "Imc1", "Imc2")}


def value_and_scale(ref, name):
    return ref["firstorder"][name] if name in ref["firstorder"] else ref["glcm_features"][name]


def deviations(ref, values, truth=None):
    """{feature class: the largest |values[name] - truth[name]| / scale over the class}; `truth` defaults to exact(ref).  A NaN on both
    sides is agreement; a scale of 0 asks for equality."""
    import mpmath as mp
    truth = exact(ref) if truth is None else truth
    out = {}
    for cls, names in CLASSES.items():
        worst = 0.0
        for name in names:
            got, want, scale = values[name], truth[name], value_and_scale(ref, name)[1]
            if mp.isnan(want) or (isinstance(got, float) and math.isnan(got)):
                dev = 0.0 if (mp.isnan(want) and math.isnan(float(got))) else float("inf")
            else:
                err = abs(mp.mpf(float(got)) - want)
                dev = float(err / mp.mpf(scale)) if scale != 0.0 else (0.0 if err == 0 else float("inf"))
            worst = max(worst, dev)
        out[cls] = worst
    return out
