"""Helpers of the RTSTRUCT tests: the numpy fp64 restatement of the `mmnn_rasterize_contours` contract (include/mmnn_sts.h), the
restatement of the millimetre -> voxel index mapping with the affine product written out term by term, a struct-based packer of
RT Structure Set files at the published element layout (through tests/_dicom_ref.py; it shares no code with synth_dicom), and the
polygons the device tests fill.  Shares no code with mmnn_sts_amd."""
import math

import numpy as np

from tests import _dicom_ref as D

RTSTRUCT = "1.2.840.10008.5.1.4.1.1.481.3"


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def edges_of(points, contours, lo, hi):
    """(x0, y0, x1, y1) of every edge of the contours [lo, hi): each contour closed from its last point back to its first."""
    parts = []
    for first, count in np.asarray(contours)[lo:hi]:
        if count < 1:
            continue
        p = np.asarray(points, dtype=np.float64)[first:first + count]
        parts.append(np.concatenate([p, np.roll(p, -1, axis=0)], axis=1))
    return np.concatenate(parts, axis=0).T if parts else np.zeros((4, 0))


def fill_ref(points, contours, slice_first, shape):
    """(mask (x, y, z) uint8, smallest |xc - i| met, smallest distance of a vertex from an integer row).  Voxel (i, j, k) is 1 iff an odd
    number of edges of slice k count for it; edge (x0, y0) -> (x1, y1) counts when (y0 <= j < y1 or y1 <= j < y0) and
    i < x0 + (j - y0) * (x1 - x0) / (y1 - y0), every operation a numpy fp64 operation of its own."""
    x, y, z = shape
    out = np.zeros(shape, dtype=np.uint8)
    ii = np.arange(x, dtype=np.float64)
    near_x, near_row = math.inf, math.inf
    pts = np.asarray(points, dtype=np.float64)
    for k in range(z):
        x0, y0, x1, y1 = edges_of(pts, contours, int(slice_first[k]), int(slice_first[k + 1]))
        if x0.size:
            near_row = min(near_row, float(np.abs(y0 - np.rint(y0)).min()))
        for j in range(y):
            fj = np.float64(j)
            cross = ((y0 <= fj) & (fj < y1)) | ((y1 <= fj) & (fj < y0))
            if not cross.any():
                continue
            a0, b0, a1, b1 = x0[cross], y0[cross], x1[cross], y1[cross]
            t = fj - b0
            t = t * (a1 - a0)
            t = t / (b1 - b0)
            xc = a0 + t
            inside = ii[:, None] < xc[None, :]
            out[:, j, k] = inside.sum(axis=1) & 1
            near_x = min(near_x, float(np.abs(xc[None, :] - ii[:, None]).min()))
    return out, near_x, near_row


def index_ref(lps, affine):
    """(n, 3) LPS millimetres -> (n, 3) continuous voxel indices of a scan with the RAS voxel-index -> mm matrix `affine`: the flip to
    RAS, then the inverse matrix applied with the product written out term by term."""
    m = np.linalg.inv(np.asarray(affine, dtype=np.float64))
    lps = np.asarray(lps, dtype=np.float64)
    rx, ry, rz = -lps[:, 0], -lps[:, 1], lps[:, 2]
    return np.stack([m[r][0] * rx + m[r][1] * ry + m[r][2] * rz + m[r][3] for r in range(3)], axis=1)


def arrays(per_slice, z):
    """The three arrays of the C-ABI from per_slice = {k: [(n, 2) polygon, ...]}."""
    points, records, slice_first, at = [], [], [0], 0
    for k in range(z):
        for poly in per_slice.get(k, []):
            poly = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
            points.append(poly)
            records.append((at, len(poly)))
            at += len(poly)
        slice_first.append(len(records))
    return (np.concatenate(points, axis=0) if points else np.zeros((0, 2)), np.asarray(records, dtype=np.int32).reshape(-1, 2),
            np.asarray(slice_first, dtype=np.int32))


# ---- polygons ------------------------------------------------------------------------------------------------------------------------
def star(centre, radius, n, rng, lobes=5, depth=0.3):
    """A smooth star polygon of n points: r(t) = radius (1 + depth cos(lobes t + phase)), seeded phase and starting angle."""
    phase, start = rng.uniform(0.0, 2.0 * math.pi, 2)
    t = start + 2.0 * math.pi * np.arange(n) / n
    r = radius * (1.0 + depth * np.cos(lobes * t + phase))
    return np.stack([centre[0] + r * np.cos(t), centre[1] + r * np.sin(t)], axis=1)


def stars(shape, seed, n=40, reach=0.42):
    """Two star polygons per slice about a seeded centre near the slice's middle, the inner one at 0.45 of the outer's radius: even-odd
    leaves a hole.  `reach`: the outer radius as a fraction of the smaller in-plane extent (above 0.5 the contours leave the grid)."""
    x, y, z = shape
    rng = np.random.default_rng([seed, x, y, z])
    per_slice = {}
    for k in range(z):
        c = ((x - 1) / 2.0 + rng.uniform(-1.0, 1.0), (y - 1) / 2.0 + rng.uniform(-1.0, 1.0))
        radius = reach * min(x, y) * rng.uniform(0.85, 1.0)
        per_slice[k] = [star(c, radius, n, rng), star(c, 0.45 * radius, max(3, n // 2), rng)]
    return per_slice


# ---- packing files -------------------------------------------------------------------------------------------------------------------
def sequence(group, elem, items, explicit=True, undefined=False):
    """A sequence element from the raw bytes of its items' data sets; `undefined`: sequence and items of undefined length."""
    if undefined:
        body = b"".join(D.el(0xFFFE, 0xE000, None, it + D.el(0xFFFE, 0xE00D, None, b""), length=D.UNDEFINED) for it in items)
        return D.el(group, elem, "SQ", body + D.el(0xFFFE, 0xE0DD, None, b""), explicit, length=D.UNDEFINED)
    return D.el(group, elem, "SQ", b"".join(D.el(0xFFFE, 0xE000, None, it) for it in items), explicit)


def number(v):
    return repr(float(v))


def rtstruct_file(rois, explicit=True, undefined=False, sop_class=RTSTRUCT, syntax=None, extra=b""):
    """`rois`: [(name, [(geometric type, (n, 3) LPS points, declared count or None), ...])].  ROI numbers are 7, 8, ... and the
    ROIContourSequence lists the ROIs in reverse order, so that the reference by number is what joins them."""
    e = lambda g, n, vr, v: D.el(g, n, vr, v, explicit)
    described, drawn = [], []
    for r, (name, contours) in enumerate(rois):
        described.append(e(0x3006, 0x0022, "IS", str(7 + r)) + e(0x3006, 0x0024, "UI", "1.2.3.9") + e(0x3006, 0x0026, "LO", name))
        items = []
        for kind, pts, declared in contours:
            pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
            items.append(e(0x3006, 0x0042, "CS", kind) + e(0x3006, 0x0046, "IS", str(len(pts) if declared is None else declared))
                         + e(0x3006, 0x0050, "DS", "\\".join(number(v) for v in pts.reshape(-1))))
        # a nested sequence the reader has no use for (ContourImageSequence) sits in front of the contours
        unused = sequence(0x3006, 0x0016, [e(0x0008, 0x1155, "UI", "1.2.3.4")], explicit, undefined)
        drawn.append(e(0x3006, 0x002A, "IS", "255\\0\\0") + sequence(0x3006, 0x0040, [unused + it for it in items], explicit, undefined)
                     + e(0x3006, 0x0084, "IS", str(7 + r)))
    body = (e(0x3006, 0x0002, "SH", "TEST") + sequence(0x3006, 0x0020, described, explicit, undefined)
            + sequence(0x3006, 0x0039, drawn[::-1], explicit, undefined))
    return D.part10({(0x0008, 0x0016): ("UI", sop_class), (0x0008, 0x0060): ("CS", "RTSTRUCT")}, None, explicit, syntax, extra=body + extra)


def square(k, lo=1.0, hi=4.0, z_of=lambda k: 2.0 * k):
    """A closed square on slice k of a grid with the identity orientation in LPS (see `LPS_AFFINE`), as (4, 3) LPS millimetres."""
    return np.array([[lo, lo, z_of(k)], [hi, lo, z_of(k)], [hi, hi, z_of(k)], [lo, hi, z_of(k)]])


# the RAS affine of a scan whose LPS millimetres are (i, j, 2 k): voxel index = (x_lps, y_lps, z / 2)
LPS_AFFINE = np.diag([-1.0, -1.0, 2.0, 1.0])
