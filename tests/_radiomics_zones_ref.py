"""numpy / scipy fp64 restatement of `mmnn_radiomics_zones` (include/mmnn_sts.h): the 26-connected zones of a bin volume, their canonical
labels, sizes and per-level counts, the six exact integers and the 16 GLSZM features, plus an mpmath evaluation of the same features from
the same exact integer tables.  The bin volume and Ng come from tests/_radiomics_ref.restate (through _radiomics_texture_ref.bin_volume).

Zones come from `scipy.ndimage.label(B == i, structure=np.ones((3, 3, 3)))` per level; `flood_fill` is an independent labelling in plain
python (a stack, the 26 offsets, bounds tested on (x, y, z)) that the CPU test holds scipy to on the small cases.

`restate` returns the tables as the device lays them out (x fastest) and, per feature, a pair (value, scale).  The scale is what a rounding
error of the evaluation is relative to: the sum of the absolute values of the terms of the feature's sum, divided by what the sum is
divided by (tests/_radiomics_ref.py derives the rule for the GLCM).

    SmallAreaEmphasis, LargeAreaEmphasis, the two GrayLevelNonUniformity, the two SizeZoneNonUniformity, Low / HighGrayLevelZoneEmphasis
    and the four joint emphases are sums of non-negative terms (counts times positive weights) over Nz or Nz^2: the scale is the value.
    ZonePercentage Nz / Np is one quotient of two exact integers: the scale is the value.
    GrayLevelVariance and ZoneVariance, sum p (i - mu)^2, have non-negative terms and are stationary in their centre (the derivative
    with respect to mu is -2 sum p (i - mu) = 0), so the centre's own rounding adds nothing at first order: the scale is the value.
    With one level (one size) every term is exactly 0 on both sides, and a scale of 0 asks for equality.
    ZoneEntropy -sum p log2(p + eps) has terms of one sign too (p + eps <= 1 up to the single case p = 1, where the one term is
    log2(1 + eps) > 0 and alone), but the terms are products with a rounded log2: the scale is sum |p log2(p + eps)|, which is |value|.
    It is kept as its own tolerance class because the device uses another log2.
"""
import math

import numpy as np

from tests import _radiomics_texture_ref as T

EPS = T.EPS
GLSZM = ("SmallAreaEmphasis", "LargeAreaEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized", "SizeZoneNonUniformity",
         "SizeZoneNonUniformityNormalized", "ZonePercentage", "GrayLevelVariance", "ZoneVariance", "ZoneEntropy", "LowGrayLevelZoneEmphasis",
         "HighGrayLevelZoneEmphasis", "SmallAreaLowGrayLevelEmphasis", "SmallAreaHighGrayLevelEmphasis", "LargeAreaLowGrayLevelEmphasis",
         "LargeAreaHighGrayLevelEmphasis")
INTEGERS = ("nz", "n_keys", "max_size", "sum_pg2", "sum_ps2", "sum_j2")
CLASSES = ("glszm_sum", "glszm_entropy")


def linear_index(shape):
    """(x, y, z) array of the device's linear index, x fastest."""
    X, Y, Z = shape
    return np.arange(X * Y * Z, dtype=np.int64).reshape(Z, Y, X).T


def flat(a):
    """An (x, y, z) array in the device's layout."""
    return np.ascontiguousarray(a.T).reshape(-1)


# ---- labelling -------------------------------------------------------------------------------------------------------------------------
def label_zones(B):
    """(labels, sizes) as (x, y, z) int64 arrays: 0 outside the ROI / 1 + the smallest linear index of the voxel's zone; the zone's voxel
    count at that smallest-index voxel, 0 elsewhere."""
    from scipy import ndimage
    lin = linear_index(B.shape)
    X, Y, Z = B.shape
    labels, sizes = np.zeros(B.shape, np.int64), np.zeros(X * Y * Z, np.int64)
    for i in np.unique(B[B > 0]):
        lab, k = ndimage.label(B == i, structure=np.ones((3, 3, 3)))
        idx = np.arange(1, k + 1)
        root = ndimage.minimum(lin, lab, index=idx).astype(np.int64)
        count = np.bincount(lab.reshape(-1), minlength=k + 1)[1:]
        on = lab > 0
        labels[on] = root[lab[on] - 1] + 1
        sizes[root] = count
    return labels, sizes.reshape(Z, Y, X).T


def flood_fill(B):
    """The same two arrays by a plain flood fill, voxels visited in ascending linear index: the first voxel of a zone met is its smallest."""
    X, Y, Z = B.shape
    labels, sizes = np.zeros(B.shape, np.int64), np.zeros(B.shape, np.int64)
    offsets = [(ex, ey, ez) for ex in (-1, 0, 1) for ey in (-1, 0, 1) for ez in (-1, 0, 1) if (ex, ey, ez) != (0, 0, 0)]
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                b = B[x, y, z]
                if b == 0 or labels[x, y, z]:
                    continue
                tag, count, stack = 1 + x + X * (y + Y * z), 0, [(x, y, z)]
                labels[x, y, z] = tag
                while stack:
                    px, py, pz = stack.pop()
                    count += 1
                    for ex, ey, ez in offsets:
                        qx, qy, qz = px + ex, py + ey, pz + ez
                        if 0 <= qx < X and 0 <= qy < Y and 0 <= qz < Z and B[qx, qy, qz] == b and not labels[qx, qy, qz]:
                            labels[qx, qy, qz] = tag
                            stack.append((qx, qy, qz))
                sizes[x, y, z] = count
    return labels, sizes


# ---- the features ------------------------------------------------------------------------------------------------------------------------
def zone_keys(B, sizes):
    """The distinct (i, j) in ascending order and their counts P: three int64 arrays."""
    root = sizes > 0
    key = B[root].astype(np.int64) << 32 | sizes[root]
    k, c = np.unique(key, return_counts=True)
    return k >> 32, k & 0xFFFFFFFF, c.astype(np.int64)


def features(I, J, C, ng, Np):
    """The 16 features [(value, scale)] from the sparse matrix."""
    Nz = float(C.sum())
    pg = np.zeros(ng)
    np.add.at(pg, I - 1, C.astype(np.float64))            # (exact: integers below 2^53)
    js, inv = np.unique(J, return_inverse=True)
    ps = np.zeros(len(js))
    np.add.at(ps, inv, C.astype(np.float64))
    i, j = np.arange(1, ng + 1, dtype=np.float64), js.astype(np.float64)
    If, Jf, P = I.astype(np.float64), J.astype(np.float64), C.astype(np.float64)
    ii, jj = If * If, Jf * Jf
    mu_i, mu_j = float((i * (pg / Nz)).sum()), float((j * (ps / Nz)).sum())
    ent = (P / Nz) * np.log2(P / Nz + EPS)
    v = [float((ps / (j * j)).sum()) / Nz, float((ps * (j * j)).sum()) / Nz, float((pg * pg).sum()) / Nz, float((pg * pg).sum()) / (Nz * Nz),
         float((ps * ps).sum()) / Nz, float((ps * ps).sum()) / (Nz * Nz), Nz / float(Np), float(((pg / Nz) * (i - mu_i) ** 2).sum()),
         float(((ps / Nz) * (j - mu_j) ** 2).sum()), -float(ent.sum()), float((pg / (i * i)).sum()) / Nz, float((pg * (i * i)).sum()) / Nz,
         float((P / (ii * jj)).sum()) / Nz, float((P * ii / jj).sum()) / Nz, float((P * jj / ii).sum()) / Nz, float((P * (ii * jj)).sum()) / Nz]
    out = [(x, abs(x)) for x in v]
    out[9] = (v[9], float(np.abs(ent).sum()))
    return out


def restate(case):
    """A case of _radiomics_cases -> dict(ref (restatement of mmnn_radiomics), flagged, labels, sizes ([N] int64, the device's layout),
    levels ([max_bins] int64), integers {name: int}, keys (I, J, C), features {name: (value, scale)})."""
    ref, B = T.bin_volume(case)
    n_vox, mb = int(np.prod(case["scan"].shape)), case["max_bins"]
    nan = (float("nan"), float("nan"))
    out = {"ref": ref, "flagged": B is None, "labels": np.zeros(n_vox, np.int64), "sizes": np.zeros(n_vox, np.int64),
           "levels": np.zeros(mb, np.int64), "integers": {k: 0 for k in INTEGERS}, "keys": None, "features": {k: nan for k in GLSZM}}
    if B is None:
        return out
    B = B.astype(np.int64)
    labels, sizes = label_zones(B)
    I, J, C = zone_keys(B, sizes)
    out["labels"], out["sizes"], out["keys"], out["bins"] = flat(labels), flat(sizes), (I, J, C), B
    np.add.at(out["levels"], I - 1, C)
    ps = {}
    for j, c in zip(J.tolist(), C.tolist()):
        ps[j] = ps.get(j, 0) + c
    out["integers"] = {"nz": int(C.sum()), "n_keys": len(C), "max_size": int(J.max()), "sum_pg2": sum(int(c) ** 2 for c in out["levels"]),
                       "sum_ps2": sum(c * c for c in ps.values()), "sum_j2": sum(j * j * c for j, c in ps.items())}
    out["features"] = dict(zip(GLSZM, features(I, J, C, ref["n_bins"], ref["n"])))
    return out


# ---- the same features in extended precision ---------------------------------------------------------------------------------------------
def exact(zn):
    """mpmath (40 digits) evaluation of the 16 features from the integer tables of `zn` = restate(case): {name: mpf}."""
    import mpmath as mp
    mp.mp.dps = 40
    eps, ln2 = mp.mpf(2) ** -52, mp.log(2)
    I, J, C = (a.tolist() for a in zn["keys"])
    Np, Nz = zn["ref"]["n"], mp.mpf(zn["integers"]["nz"])
    pg = {i + 1: int(c) for i, c in enumerate(zn["levels"]) if c}
    ps = {}
    for j, c in zip(J, C):
        ps[j] = ps.get(j, 0) + c
    mu_i = mp.fsum(i * mp.mpf(c) for i, c in pg.items()) / Nz
    mu_j = mp.fsum(j * mp.mpf(c) for j, c in ps.items()) / Nz
    g2, s2 = mp.mpf(sum(c * c for c in pg.values())), mp.mpf(sum(c * c for c in ps.values()))
    nz = list(zip(I, J, C))
    v = [mp.fsum(mp.mpf(c) / (j * j) for j, c in ps.items()) / Nz, mp.fsum(mp.mpf(c) * (j * j) for j, c in ps.items()) / Nz, g2 / Nz, g2 / (Nz * Nz),
         s2 / Nz, s2 / (Nz * Nz), Nz / Np, mp.fsum(mp.mpf(c) / Nz * (i - mu_i) ** 2 for i, c in pg.items()),
         mp.fsum(mp.mpf(c) / Nz * (j - mu_j) ** 2 for j, c in ps.items()),
         -mp.fsum((mp.mpf(c) / Nz) * mp.log(mp.mpf(c) / Nz + eps) / ln2 for _, _, c in nz),
         mp.fsum(mp.mpf(c) / (i * i) for i, c in pg.items()) / Nz, mp.fsum(mp.mpf(c) * (i * i) for i, c in pg.items()) / Nz,
         mp.fsum(mp.mpf(c) / (i * i * j * j) for i, j, c in nz) / Nz, mp.fsum(mp.mpf(c) * (i * i) / (j * j) for i, j, c in nz) / Nz,
         mp.fsum(mp.mpf(c) * (j * j) / (i * i) for i, j, c in nz) / Nz, mp.fsum(mp.mpf(c) * (i * i * j * j) for i, j, c in nz) / Nz]
    return dict(zip(GLSZM, v))


def class_of(name):
    return "glszm_entropy" if name.endswith("Entropy") else "glszm_sum"


def deviations(zn, values, truth):
    """{tolerance class: the largest |values[name] - truth[name]| / scale over the class}.  A scale of 0 asks for equality."""
    import mpmath as mp
    out = {k: 0.0 for k in CLASSES}
    for name, (_, scale) in zn["features"].items():
        got, want = float(values[name]), truth[name]
        if math.isnan(got):
            dev = float("inf")
        else:
            err = abs(mp.mpf(got) - want)
            dev = float(err / mp.mpf(scale)) if scale != 0.0 else (0.0 if err == 0 else float("inf"))
        k = class_of(name)
        out[k] = max(out[k], dev)
    return out
