"""Helpers of the mask-resample tests: the fp64 numpy restatement of the `mmnn_resample_mask` contract (include/mmnn_sts.h) -- what
`sitk.Resample(mask, image)` with its defaults followed by upstream's rebinarisation computes -- the preconditions under which a
byte-for-byte comparison with it is meaningful, affine builders, the cases, and a struct-based reader / packer of the NIfTI-1 geometry
fields at the published offsets.  Shares no code with mmnn_sts_amd."""
import gzip
import math
import struct

import numpy as np

from tests import _ingest_ref as R

MARGIN = 1e-9


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def coordinates(scan_shape, T):
    """c[r] (x, y, z) float64: the continuous mask index of every scan voxel, c_r = T[r][0] i + T[r][1] j + T[r][2] k + T[r][3]."""
    T = np.asarray(T, dtype=np.float64)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in scan_shape], indexing="ij")
    return [T[r, 0] * i + T[r, 1] * j + T[r, 2] * k + T[r, 3] for r in range(3)]


def resample_ref(mask, scan_shape, T, threshold=0.5, slope=1.0, inter=0.0):
    """(bytes uint8 (x, y, z), m float64 (NaN outside the mask's grid), c): identity transform, linear interpolator, default pixel
    value 0, then `> threshold`.  Inside is ITK's buffer test -0.5 <= c_r < m_r - 0.5; the eight neighbour indices floor(c_r),
    floor(c_r) + 1 are clamped to the grid; the blend is the eight-term sum of weight * scaled voxel."""
    v = R.fdata(mask, slope, inter)
    dims = v.shape
    c = coordinates(scan_shape, T)
    inside = np.ones(tuple(scan_shape), dtype=bool)
    for r in range(3):
        inside &= (c[r] >= -0.5) & (c[r] < dims[r] - 0.5)
    f = [np.floor(np.clip(c[r], -1.0, dims[r])) for r in range(3)]
    w = [np.where(inside, c[r] - f[r], 0.0) for r in range(3)]
    lo = [np.clip(f[r].astype(np.int64), 0, dims[r] - 1) for r in range(3)]
    hi = [np.clip(f[r].astype(np.int64) + 1, 0, dims[r] - 1) for r in range(3)]
    acc = np.zeros(tuple(scan_shape), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    weight = (w[0] if dx else 1.0 - w[0]) * (w[1] if dy else 1.0 - w[1]) * (w[2] if dz else 1.0 - w[2])
                    acc += weight * v[(hi[0] if dx else lo[0]), (hi[1] if dy else lo[1]), (hi[2] if dz else lo[2])]
        m = np.where(inside, acc, np.nan)
        out = (inside & (acc > threshold)).astype(np.uint8)
    return out, m, c


def margins(out, m, c, mask_shape, threshold):
    """(smallest |m - threshold| over the inside voxels, smallest distance of a coordinate from -0.5 or m_r - 0.5)."""
    with np.errstate(invalid="ignore"):
        d = np.abs(m - threshold)
    value = float(np.nanmin(d)) if np.isfinite(d).any() else math.inf
    edge = min(float(min(np.abs(c[r] + 0.5).min(), np.abs(c[r] - (mask_shape[r] - 0.5)).min())) for r in range(3))
    return value, edge


def assert_comparable(out, m, c, mask_shape, threshold, label="", partial=True):
    """The preconditions of a byte-for-byte comparison, on the restatement alone.  The bound is derived, not measured: an fp64 trilinear
    blend of values <= V errs by <~ 2e-15 V and a coordinate by <~ 1e-13 voxel at these extents, four orders of magnitude below 1e-9."""
    value, edge = margins(out, m, c, mask_shape, threshold)
    print(f"{label}: {int(out.sum())} of {out.size} voxels set; margin to the threshold {value:.3e}, to the grid's boundary {edge:.3e}")
    assert value >= MARGIN * max(1.0, abs(threshold)), f"{label}: a blend lies within {value:.3e} of the threshold"
    assert edge >= MARGIN, f"{label}: a coordinate lies within {edge:.3e} of the mask grid's boundary"
    if partial:
        assert 0 < int(out.sum()) < out.size, f"{label}: the resampled mask is empty or full"


# ---- affines ---------------------------------------------------------------------------------------------------------------------
def rot(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    return {"x": np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]),
            "y": np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]),
            "z": np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])}[axis]


def affine(rotations, spacing, offset):
    """A = [R diag(spacing) | t], R the product of the (axis, angle) rotations in the order given."""
    Rm = np.eye(3)
    for axis, angle in rotations:
        Rm = Rm @ rot(axis, angle)
    A = np.eye(4)
    A[:3, :3] = Rm @ np.diag(np.asarray(spacing, dtype=np.float64))
    A[:3, 3] = offset
    return A


def index_map(scan_affine, mask_affine):
    return (np.linalg.inv(np.asarray(mask_affine, dtype=np.float64)) @ np.asarray(scan_affine, dtype=np.float64))[:3]


_A_SCAN = ((), (1.0, 1.1, 2.5), (-10.0, -9.0, -20.0))
_A_MASK = ((("z", 0.21), ("x", -0.13)), (1.7, 1.3, 2.9), (-9.3, -12.1, -17.7))
# name -> (scan grid, mask grid, scan affine (rotations, spacing, offset), mask affine)
CASES = {
    "A": ((20, 18, 16), (13, 17, 11), _A_SCAN, _A_MASK),
    "B": ((70, 5, 33), (13, 17, 11), ((("y", 0.1),), (0.31, 3.3, 0.9), (-10.2, -8.0, -15.1)), _A_MASK),      # x % 4 != 0, an axis < 8
    "C": ((20, 18, 16), (9, 8, 7), _A_SCAN, ((), (1.0, 1.1, 2.5), (-5.37, -4.2, -11.9))),                     # a cropped mask, same directions
    "D": ((20, 18, 16), (13, 17, 11), _A_SCAN, ((("z", 0.21),), (-1.7, 1.3, 2.9), (11.3, -12.1, -17.7))),     # a left-handed mask
    "E": ((133, 70, 9), (40, 36, 12), ((("z", 0.05),), (0.4, 0.55, 3.1), (-30.1, -20.3, -14.2)),              # > one wave along x, tails everywhere
          ((("z", -0.11), ("y", 0.07)), (1.1, 0.9, 2.3), (-22.7, -15.9, -13.3))),
}


def case(name):
    """(scan grid, mask grid, scan affine, mask affine, T)."""
    scan_shape, mask_shape, sa, ma = CASES[name]
    SA, MA = affine(*sa), affine(*ma)
    return scan_shape, mask_shape, SA, MA, index_map(SA, MA)


def ellipsoid(shape, seed, holes=0.03, dtype="u1", value=1):
    """An ellipsoid about the grid's centre (semi-axes 0.38 of the extents) with a seeded fraction of its voxels cleared."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    m = sum(((x - (n - 1) / 2.0) / (0.38 * n)) ** 2 for x, n in zip(g, shape)) <= 1.0
    m &= rng.random(shape) >= holes
    return (m * value).astype(np.dtype(dtype))


# ---- NIfTI-1 geometry by struct, at the published offsets -----------------------------------------------------------------------------
def parse_affine(buf, bo="<"):
    """sform when sform_code@254 > 0 (srow_x/y/z@280/296/312); else qform when qform_code@252 > 0 (quatern_b/c/d@256, qoffset@268,
    pixdim@76, qfac = pixdim[0], 0 read as +1); else None."""
    qform_code, sform_code = struct.unpack_from(bo + "2h", buf, 252)
    A = np.eye(4)
    if sform_code > 0:
        A[:3] = np.asarray(struct.unpack_from(bo + "12f", buf, 280), dtype=np.float64).reshape(3, 4)
        return A
    if qform_code > 0:
        A[:3, :3] = quaternion_rotation(*struct.unpack_from(bo + "3f", buf, 256))
        pixdim = struct.unpack_from(bo + "4f", buf, 76)
        qfac = -1.0 if pixdim[0] < 0 else 1.0
        A[:3, :3] = A[:3, :3] * np.array([pixdim[1], pixdim[2], pixdim[3] * qfac], dtype=np.float64)
        A[:3, 3] = struct.unpack_from(bo + "3f", buf, 268)
        return A
    return None


def quaternion_rotation(b, c, d):
    """The NIfTI-1 standard's rotation of the unit quaternion (a, b, c, d), a = sqrt(max(0, 1 - b^2 - c^2 - d^2))."""
    b, c, d = float(b), float(c), float(d)
    a = math.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
    return np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                     [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                     [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]])


def pack_geometry(raw, code, qform=None, sform=None, byteorder="<"):
    """File bytes as `_ingest_ref.pack_nifti` writes them, plus the geometry: `qform` = (qform_code, (b, c, d), (qoffset x, y, z),
    (pixdim 0..3)); `sform` = (sform_code, 3x4 rows).  Both None: both codes 0."""
    h = bytearray(R.pack_nifti(raw, code, byteorder=byteorder))
    bo = byteorder
    if qform is not None:
        qcode, quatern, qoffset, pixdim = qform
        struct.pack_into(bo + "h", h, 252, qcode)
        struct.pack_into(bo + "3f", h, 256, *quatern)
        struct.pack_into(bo + "3f", h, 268, *qoffset)
        struct.pack_into(bo + "4f", h, 76, *pixdim)
    if sform is not None:
        scode, rows = sform
        struct.pack_into(bo + "h", h, 254, scode)
        struct.pack_into(bo + "12f", h, 280, *np.asarray(rows, dtype=np.float64)[:3].reshape(-1))
    return bytes(h)


def identity_header(shape, code, slope=1.0, inter=0.0):
    """The 352 bytes the writer emitted before it knew geometry, field by field: sizeof_hdr 348; dim; datatype, bitpix; pixdim all 1;
    vox_offset 352, scl_slope, scl_inter; xyzt_units 2 (mm); qform_code 0, sform_code 2; the identity in srow_x/y/z; magic n+1."""
    h = bytearray(352)
    struct.pack_into("<i", h, 0, 348)
    struct.pack_into("<8h", h, 40, len(shape), *shape, *([1] * (7 - len(shape))))
    struct.pack_into("<2h", h, 70, code, R.BITPIX[code])
    struct.pack_into("<8f", h, 76, *([1.0] * 8))
    struct.pack_into("<3f", h, 108, 352.0, slope, inter)
    struct.pack_into("<b", h, 123, 2)
    struct.pack_into("<2h", h, 252, 0, 2)
    struct.pack_into("<12f", h, 280, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    h[344:348] = b"n+1\0"
    return bytes(h)


def file_bytes(path):
    path = str(path)
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        return f.read()


def strip_geometry(path):
    """Rewrite the file with qform_code = sform_code = 0."""
    path = str(path)
    h = bytearray(file_bytes(path))
    struct.pack_into("<2h", h, 252, 0, 0)
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(bytes(h))
