"""numpy fp64 restatement of `mmnn_radiomics_texture` (include/mmnn_sts.h): the run-length (GLRLM), dependence (GLDM) and neighbouring
grey-tone difference (NGTDM) tables of a bin volume and their 16 + 14 + 5 features, plus an mpmath evaluation of the same features from
the same exact integer tables.  The bin volume and Ng come from tests/_radiomics_ref.restate.

`restate` returns the four integer tables as the device lays them out and, per feature, a pair (value, scale).  The scale is what a
rounding error of the evaluation is relative to, as the docstring of tests/_radiomics_ref.py derives it for the GLCM: the sum of the
absolute values of the terms of the feature's sum (divided by what the sum is divided by).

    Every GLRLM / GLDM sum but the entropy has non-negative terms, so its scale is its value; the two variances are stationary in their
    centre (mu_g, mu_r), so the centre's own rounding adds nothing at first order.  The entropies take sum |p log2(p + eps)|.
    The NGTDM features are products and quotients of sums of non-negative terms whose inputs s_i are themselves rounded sums (26 terms
    s[i][c] / c): a quotient takes the scale of the numerator over the denominator plus |value| for a denominator that is a rounded
    sum, and every level of rounded positive sums below adds |value| once more: Coarseness 1 / S(s) -> 2 |v|;  Contrast A B(s) -> 3 |v|;
    Busyness S(s) / D -> 3 |v|;  Complexity S(s) / Nvp -> 2 |v|;  Strength A / S(s) -> 3 |v|.

A GLRLM feature, averaged over the 13 directions, takes the average of the directions' scales.
"""
import math

import numpy as np

from tests import _radiomics_ref as R

EPS = R.EPS
DIRECTIONS = R.DIRECTIONS
GLRLM = ("ShortRunEmphasis", "LongRunEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized", "RunLengthNonUniformity",
         "RunLengthNonUniformityNormalized", "RunPercentage", "GrayLevelVariance", "RunVariance", "RunEntropy", "LowGrayLevelRunEmphasis",
         "HighGrayLevelRunEmphasis", "ShortRunLowGrayLevelEmphasis", "ShortRunHighGrayLevelEmphasis", "LongRunLowGrayLevelEmphasis",
         "LongRunHighGrayLevelEmphasis")
GLDM = ("SmallDependenceEmphasis", "LargeDependenceEmphasis", "GrayLevelNonUniformity", "DependenceNonUniformity",
        "DependenceNonUniformityNormalized", "GrayLevelVariance", "DependenceVariance", "DependenceEntropy", "LowGrayLevelEmphasis",
        "HighGrayLevelEmphasis", "SmallDependenceLowGrayLevelEmphasis", "SmallDependenceHighGrayLevelEmphasis",
        "LargeDependenceLowGrayLevelEmphasis", "LargeDependenceHighGrayLevelEmphasis")
NGTDM = ("Coarseness", "Contrast", "Busyness", "Complexity", "Strength")
_GLDM_FROM = (0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15)          # the dependence class is the run-length one without two features
NGTDM_LEVELS = {"Coarseness": 2.0, "Contrast": 3.0, "Busyness": 3.0, "Complexity": 2.0, "Strength": 3.0}
CLASSES = ("glrlm_sum", "glrlm_entropy", "gldm_sum", "gldm_entropy", "ngtdm")


def bin_volume(case):
    """(restatement of mmnn_radiomics, bin volume (x, y, z) with 0 outside the ROI or None with a flag set) of a case of _radiomics_cases."""
    with np.errstate(all="ignore"):
        ref = R.restate(case["scan"], case["mask"], case["bin_width"], case["max_bins"], case["scan_scale"], case["mask_scale"])
    flagged = ref["empty"] or ref["nonfinite"] or ref["overflow"]
    return ref, (None if flagged else ref["bins"])


# ---- the four tables ---------------------------------------------------------------------------------------------------------------------
def count_glrlm(B, max_bins):
    """(13, max_bins, L) int64.  Along direction d a voxel starts a run when its predecessor is out of the volume, out of the ROI or in
    another bin, and ends one when its successor is.  On a line of the direction starts and ends alternate, so in the order (line,
    position on the line) the k-th start and the k-th end belong to one run."""
    X, Y, Z = B.shape
    L = max(B.shape)
    P = np.zeros((13, max_bins, L), dtype=np.int64)
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    pad = np.zeros((X + 2, Y + 2, Z + 2), dtype=np.int64)
    pad[1:-1, 1:-1, 1:-1] = B
    for d, (dz, dy, dx) in enumerate(DIRECTIONS):
        prev = pad[1 - dx:1 - dx + X, 1 - dy:1 - dy + Y, 1 - dz:1 - dz + Z]
        nxt = pad[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
        start, end = (B > 0) & (prev != B), (B > 0) & (nxt != B)
        t = z if dz else (y if dy else x)                # the position on the line: the first non-zero component is +1
        line = (((z - t * dz) + L) * (3 * L + 1) + (y - t * dy) + L) * (3 * L + 1) + (x - t * dx) + L
        key = line * L + t
        ks, ke = key[start], key[end]
        order = np.argsort(ks, kind="stable")
        length = np.sort(ke) - ks[order] + 1
        np.add.at(P[d], (B[start][order] - 1, length - 1), 1)
    return P


def count_glrlm_by_walking(B, max_bins):
    """The same table by plain loops: every ROI voxel that starts a run walks it."""
    X, Y, Z = B.shape
    P = np.zeros((13, max_bins, max(B.shape)), dtype=np.int64)
    inside = lambda x, y, z: 0 <= x < X and 0 <= y < Y and 0 <= z < Z
    for d, (dz, dy, dx) in enumerate(DIRECTIONS):
        for x, y, z in np.argwhere(B > 0):
            b = B[x, y, z]
            if inside(x - dx, y - dy, z - dz) and B[x - dx, y - dy, z - dz] == b:
                continue
            n = 1
            while inside(x + n * dx, y + n * dy, z + n * dz) and B[x + n * dx, y + n * dy, z + n * dz] == b:
                n += 1
            P[d, b - 1, n - 1] += 1
    return P


def count_neighbourhood(B, max_bins):
    """gldm, ngtdm_n, ngtdm_s: (max_bins, 27) int64 each."""
    X, Y, Z = B.shape
    pad = np.zeros((X + 2, Y + 2, Z + 2), dtype=np.int64)
    pad[1:-1, 1:-1, 1:-1] = B
    c, same, tot = (np.zeros(B.shape, dtype=np.int64) for _ in range(3))
    for ex in (-1, 0, 1):
        for ey in (-1, 0, 1):
            for ez in (-1, 0, 1):
                if (ex, ey, ez) == (0, 0, 0):
                    continue
                nb = pad[1 + ex:1 + ex + X, 1 + ey:1 + ey + Y, 1 + ez:1 + ez + Z]
                c += nb > 0
                tot += nb
                same += nb == B
    roi = B > 0
    gldm, n, s = (np.zeros((max_bins, 27), dtype=np.int64) for _ in range(3))
    np.add.at(gldm, (B[roi] - 1, same[roi]), 1)
    np.add.at(n, (B[roi] - 1, c[roi]), 1)
    np.add.at(s, (B[roi] - 1, c[roi]), np.abs(B[roi] * c[roi] - tot[roi]))
    return gldm, n, s


# ---- the features ------------------------------------------------------------------------------------------------------------------------
def matrix_features(P, Np):
    """(ng, J) counts -> the 16 run-length features [(value, scale)] in the order of GLRLM; None for an empty matrix."""
    Nr = float(P.sum())
    if Nr == 0.0:
        return None
    ng, J = P.shape
    P = P.astype(np.float64)
    i, j = np.arange(1, ng + 1, dtype=np.float64), np.arange(1, J + 1, dtype=np.float64)
    ii, jj = (i * i)[:, None], (j * j)[None, :]
    pg, pr = P.sum(axis=1), P.sum(axis=0)
    mu_g, mu_r = float((i * (pg / Nr)).sum()), float((j * (pr / Nr)).sum())
    ent = (P / Nr) * np.log2(P / Nr + EPS)
    v = [float((pr / (j * j)).sum()) / Nr, float((pr * (j * j)).sum()) / Nr, float((pg * pg).sum()) / Nr, float((pg * pg).sum()) / (Nr * Nr),
         float((pr * pr).sum()) / Nr, float((pr * pr).sum()) / (Nr * Nr), Nr / float(Np), float(((pg / Nr) * (i - mu_g) ** 2).sum()),
         float(((pr / Nr) * (j - mu_r) ** 2).sum()), -float(ent.sum()), float((pg / (i * i)).sum()) / Nr, float((pg * (i * i)).sum()) / Nr,
         float((P / (ii * jj)).sum()) / Nr, float((P * ii / jj).sum()) / Nr, float((P * jj / ii).sum()) / Nr, float((P * (ii * jj)).sum()) / Nr]
    out = [(x, abs(x)) for x in v]
    out[9] = (v[9], float(np.abs(ent).sum()))
    return out


def ngtdm_features(n, s):
    """(ng, 27) n and s -> the five features [(value, scale)]; NaN when no voxel has a neighbour."""
    ni = n[:, 1:].sum(axis=1)
    si = np.zeros(len(ni))
    for c in range(1, 27):                               # in this order, as the device adds them
        si = si + s[:, c].astype(np.float64) / float(c)
    Nvp = float(ni.sum())
    if Nvp == 0.0:
        return [(float("nan"), float("nan"))] * 5
    on = ni > 0
    Ngp = int(on.sum())
    lv = np.arange(1, len(ni) + 1, dtype=np.float64)[on]
    p, sv = ni[on] / Nvp, si[on]
    S, T = float((p * sv).sum()), float(sv.sum())
    dl = lv[:, None] - lv[None, :]
    pi, pj = p[:, None], p[None, :]
    A = float((pi * pj * (dl * dl)).sum())
    D = float(np.abs(lv[:, None] * pi - lv[None, :] * pj).sum())
    C = float((np.abs(dl) * (pi * sv[:, None] + pj * sv[None, :]) / (pi + pj)).sum())
    Q = float(((pi + pj) * (dl * dl)).sum())
    v = [1.0e6 if S == 0.0 else 1.0 / S, 0.0 if Ngp == 1 else (A / (Ngp * (Ngp - 1.0))) * (T / Nvp), 0.0 if D == 0.0 else S / D, C / Nvp,
         0.0 if T == 0.0 else Q / T]
    return [(x, NGTDM_LEVELS[k] * abs(x)) for k, x in zip(NGTDM, v)]


def restate(case):
    """A case of _radiomics_cases -> dict(ref (restatement of mmnn_radiomics), flagged, glrlm, gldm, ngtdm_n, ngtdm_s (int64, the device's
    layout), features {class: {name: (value, scale)}})."""
    ref, B = bin_volume(case)
    mb, L = case["max_bins"], max(case["scan"].shape)
    nan = (float("nan"), float("nan"))
    out = {"ref": ref, "flagged": B is None, "glrlm": np.zeros((13, mb, L), np.int64), "gldm": np.zeros((mb, 27), np.int64),
           "ngtdm_n": np.zeros((mb, 27), np.int64), "ngtdm_s": np.zeros((mb, 27), np.int64),
           "features": {"glrlm": {k: nan for k in GLRLM}, "gldm": {k: nan for k in GLDM}, "ngtdm": {k: nan for k in NGTDM}}}
    if B is None:
        return out
    ng, n = ref["n_bins"], ref["n"]
    out["glrlm"] = count_glrlm(B, mb)
    out["gldm"], out["ngtdm_n"], out["ngtdm_s"] = count_neighbourhood(B, mb)
    per = [matrix_features(out["glrlm"][d, :ng], n) for d in range(13)]
    assert all(f is not None for f in per)               # no direction is empty when n > 0
    out["features"]["glrlm"] = {k: (sum(f[q][0] for f in per) / 13.0, sum(f[q][1] for f in per) / 13.0) for q, k in enumerate(GLRLM)}
    dm = matrix_features(out["gldm"][:ng], n)
    out["features"]["gldm"] = {k: dm[q] for k, q in zip(GLDM, _GLDM_FROM)}
    out["features"]["ngtdm"] = dict(zip(NGTDM, ngtdm_features(out["ngtdm_n"][:ng], out["ngtdm_s"][:ng])))
    return out


# ---- the same features in extended precision -------------------------------------------------------------------------------------------------
def _exact_matrix(P, Np, mp):
    eps, ln2 = mp.mpf(2) ** -52, mp.log(2)
    Nr = mp.mpf(int(P.sum()))
    pg, pr = [int(c) for c in P.sum(axis=1)], [int(c) for c in P.sum(axis=0)]
    nz = [(int(i) + 1, int(j) + 1, int(P[i, j])) for i, j in zip(*np.nonzero(P))]
    mu_g = mp.fsum(i * mp.mpf(c) for i, c in enumerate(pg, 1)) / Nr
    mu_r = mp.fsum(j * mp.mpf(c) for j, c in enumerate(pr, 1)) / Nr
    by_c = {}
    for _, _, c in nz:
        by_c[c] = by_c.get(c, 0) + 1
    g2, r2 = mp.fsum(mp.mpf(c) ** 2 for c in pg), mp.fsum(mp.mpf(c) ** 2 for c in pr)
    return [mp.fsum(mp.mpf(c) / (j * j) for j, c in enumerate(pr, 1)) / Nr, mp.fsum(mp.mpf(c) * (j * j) for j, c in enumerate(pr, 1)) / Nr,
            g2 / Nr, g2 / (Nr * Nr), r2 / Nr, r2 / (Nr * Nr), Nr / Np, mp.fsum(mp.mpf(c) / Nr * (i - mu_g) ** 2 for i, c in enumerate(pg, 1)),
            mp.fsum(mp.mpf(c) / Nr * (j - mu_r) ** 2 for j, c in enumerate(pr, 1)),
            -mp.fsum(k * (mp.mpf(c) / Nr) * mp.log(mp.mpf(c) / Nr + eps) / ln2 for c, k in by_c.items()),
            mp.fsum(mp.mpf(c) / (i * i) for i, c in enumerate(pg, 1)) / Nr, mp.fsum(mp.mpf(c) * (i * i) for i, c in enumerate(pg, 1)) / Nr,
            mp.fsum(mp.mpf(c) / (i * i * j * j) for i, j, c in nz) / Nr, mp.fsum(mp.mpf(c) * (i * i) / (j * j) for i, j, c in nz) / Nr,
            mp.fsum(mp.mpf(c) * (j * j) / (i * i) for i, j, c in nz) / Nr, mp.fsum(mp.mpf(c) * (i * i * j * j) for i, j, c in nz) / Nr]


def exact(tex):
    """mpmath (40 digits) evaluation of the 35 features from the integer tables of `tex` = restate(case): {class: {name: mpf}}."""
    import mpmath as mp
    mp.mp.dps = 40
    ng, Np = tex["ref"]["n_bins"], tex["ref"]["n"]
    per = [_exact_matrix(tex["glrlm"][d, :ng], Np, mp) for d in range(13)]
    out = {"glrlm": {k: mp.fsum(f[q] for f in per) / 13 for q, k in enumerate(GLRLM)}}
    dm = _exact_matrix(tex["gldm"][:ng], Np, mp)
    out["gldm"] = {k: dm[q] for k, q in zip(GLDM, _GLDM_FROM)}
    n, s = tex["ngtdm_n"][:ng], tex["ngtdm_s"][:ng]
    ni = [int(c) for c in n[:, 1:].sum(axis=1)]
    Nvp = sum(ni)
    if Nvp == 0:
        out["ngtdm"] = {k: mp.nan for k in NGTDM}
        return out
    lv = [i + 1 for i, c in enumerate(ni) if c > 0]
    p = {i: mp.mpf(ni[i - 1]) / Nvp for i in lv}
    sv = {i: mp.fsum(mp.mpf(int(s[i - 1, c])) / c for c in range(1, 27)) for i in lv}
    S, T, Ngp = mp.fsum(p[i] * sv[i] for i in lv), mp.fsum(sv[i] for i in lv), len(lv)
    A = mp.fsum(p[i] * p[j] * (i - j) ** 2 for i in lv for j in lv)
    D = mp.fsum(abs(i * p[i] - j * p[j]) for i in lv for j in lv)
    C = mp.fsum(abs(i - j) * (p[i] * sv[i] + p[j] * sv[j]) / (p[i] + p[j]) for i in lv for j in lv)
    Q = mp.fsum((p[i] + p[j]) * (i - j) ** 2 for i in lv for j in lv)
    out["ngtdm"] = {"Coarseness": mp.mpf(10) ** 6 if S == 0 else 1 / S, "Contrast": mp.mpf(0) if Ngp == 1 else A / (Ngp * (Ngp - 1)) * (T / Nvp),
                    "Busyness": mp.mpf(0) if D == 0 else S / D, "Complexity": C / Nvp, "Strength": mp.mpf(0) if T == 0 else Q / T}
    return out


def class_of(cls, name):
    if cls == "ngtdm":
        return "ngtdm"
    return f"{cls}_entropy" if name.endswith("Entropy") else f"{cls}_sum"


def deviations(tex, values, truth):
    """{tolerance class: the largest |values[cls][name] - truth[cls][name]| / scale over the class}.  A NaN on both sides is agreement; a
    scale of 0 asks for equality."""
    import mpmath as mp
    out = {k: 0.0 for k in CLASSES}
    for cls, feats in tex["features"].items():
        for name, (_, scale) in feats.items():
            got, want = float(values[cls][name]), truth[cls][name]
            if mp.isnan(want) or math.isnan(got):
                dev = 0.0 if (mp.isnan(want) and math.isnan(got)) else float("inf")
            else:
                err = abs(mp.mpf(got) - want)
                dev = float(err / mp.mpf(scale)) if scale != 0.0 else (0.0 if err == 0 else float("inf"))
            k = class_of(cls, name)
            out[k] = max(out[k], dev)
    return out
