"""Helpers of the NIfTI / ingest tests: the fp64 restatement of what upstream's image datasets do per volume (the reference the device
ingest is compared against), seeded case builders, and a struct-based NIfTI-1 parser / packer that shares no code with
mmnn_sts_amd.data.nifti (the reader and writer are checked against the published offsets, never against each other)."""
import gzip
import math
import struct
from fractions import Fraction

import numpy as np

SIZE = 64
NP_OF_CODE = {2: "u1", 4: "i2", 8: "i4", 16: "f4", 64: "f8", 256: "i1", 512: "u2", 768: "u4"}
BITPIX = {2: 8, 4: 16, 8: 32, 16: 32, 64: 64, 256: 8, 512: 16, 768: 32, 128: 24, 32: 64}
CODE_OF_NP = {np.dtype(v): k for k, v in NP_OF_CODE.items()}


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def fdata(raw, slope=1.0, inter=0.0):
    """nibabel's get_fdata(): float64 `raw * slope + inter` (slope / inter are the header's float32 values widened); unscaled when the
    slope is 0, NaN or infinite; a non-finite inter is 0."""
    a = np.asarray(raw).astype(np.float64)
    slope, inter = float(np.float32(slope)), float(np.float32(inter))
    if slope == 0.0 or not math.isfinite(slope):
        return a
    if not math.isfinite(inter):
        inter = 0.0
    if slope == 1.0 and inter == 0.0:
        return a
    return a * slope + inter


def area_windows(m, size=SIZE):
    """[floor(a m / size), ceil((a + 1) m / size)) for a in 0..size-1: adaptive average pooling's windows."""
    return [((a * m) // size, -((-(a + 1) * m) // size)) for a in range(size)]


def area_resize_fp64(v, size=SIZE):
    """Separable window means along the three axes, in float64."""
    for axis in range(3):
        v = np.stack([v.take(range(b, e), axis=axis).mean(axis=axis) for b, e in area_windows(v.shape[axis], size)], axis=axis)
    return v


def masked_volume(scan, mask, scan_scaling=(1.0, 0.0), mask_scaling=(1.0, 0.0)):
    return fdata(scan, *scan_scaling) * fdata(mask, *mask_scaling)


def ingest_ref(scan, mask, scan_scaling=(1.0, 0.0), mask_scaling=(1.0, 0.0)):
    """(plane float64 (64,64,64), extents (Mx, My, Mz), v): image * mask in float64, every all-zero slice dropped along each axis
    (np.any flags, boolean indexing; NaN counts as non-zero), area resize to 64^3.  An empty result -> zeros and (0, 0, 0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = masked_volume(scan, mask, scan_scaling, mask_scaling)
        nz = ~(v == 0)
        keep = [np.any(nz, axis=tuple(a for a in range(3) if a != axis)) for axis in range(3)]
        ext = tuple(int(k.sum()) for k in keep)
        if min(ext) == 0:
            return np.zeros((SIZE,) * 3), (0, 0, 0), v
        c = v[keep[0]][:, keep[1]][:, :, keep[2]]
        return area_resize_fp64(c), ext, v


def tolerance(v):
    """2 * 2^-24 * max|v| over the finite voxels: the one visible error of the device result is the final rounding of a mean whose
    magnitude is at most max|v| (half a unit); summation order in fp64 adds ~1e-16 relative; 2 units allowed."""
    f = np.abs(v[np.isfinite(v)])
    return 2.0 * 2.0 ** -24 * float(f.max() if f.size else 0.0)


def largest_window(ext, size=SIZE):
    return int(np.prod([max(e - b for b, e in area_windows(m, size)) for m in ext]))


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------
def random_scan(rng, shape, code):
    """Voxels of NIfTI type `code`, none of them zero (so that emptiness comes from the mask alone)."""
    dt = np.dtype(NP_OF_CODE[code])
    if dt.kind == "f":
        a = rng.standard_normal(shape) * 300.0
        a[a == 0] = 1.0
        return a.astype(dt)
    info = np.iinfo(dt)
    a = rng.integers(max(info.min, -30000), min(info.max, 30000) + 1, shape, dtype=np.int64)
    a[a == 0] = 1
    return a.astype(dt)


def box_mask(shape, lo, hi, holes=((), (), ()), dtype="u1", value=1):
    """1 inside the box [lo, hi) except on the hole slices (absolute indices, per axis)."""
    m = np.zeros(shape, dtype=np.dtype(dtype))
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value
    for axis, idx in enumerate(holes):
        for i in idx:
            sl = [slice(None)] * 3
            sl[axis] = i
            m[tuple(sl)] = 0
    return m


def exact_zero_raws(slope32, inters=(-3.0, -5.0, -6.0, -7.0, -9.0, -10.0, -11.0)):
    """(inter, raws): the first inter of `inters` for which float64 raws r exist with fl(r * slope) == -inter exactly although the exact
    product differs from -inter -- the rounded multiply followed by the rounded add gives 0 there, a fused multiply-add leaves a
    residue -- and those raws (the neighbours of -inter / slope are searched)."""
    s = float(np.float32(slope32))
    for inter in inters:
        t = -float(np.float32(inter))
        cand = [t / s]
        for _ in range(8):
            cand = [np.nextafter(cand[0], -np.inf)] + cand + [np.nextafter(cand[-1], np.inf)]
        out = [float(r) for r in cand if float(r) * s == t and Fraction(float(r)) * Fraction(s) != Fraction(t)]
        if out:
            return float(inter), np.asarray(out)
    raise AssertionError("no raw value found whose rounded product hits -inter")


# ---- NIfTI-1 by struct, at the published offsets ------------------------------------------------------------------------------------
def pack_nifti(raw, code, slope=1.0, inter=0.0, byteorder="<", magic=b"n+1\0", dim=None, vox_offset=352.0, truncate=0, bitpix=None):
    """File bytes of a single-file NIfTI-1 volume: `raw` (x, y, z[, ...]) written x fastest in `byteorder`."""
    raw = np.asarray(raw)
    bo = byteorder
    h = bytearray(int(vox_offset))
    struct.pack_into(bo + "i", h, 0, 348)                                                   # sizeof_hdr
    d = list(dim) if dim is not None else [raw.ndim, *raw.shape]
    struct.pack_into(bo + "8h", h, 40, *(d + [1] * (8 - len(d))))                           # dim
    struct.pack_into(bo + "h", h, 70, code)                                                 # datatype
    struct.pack_into(bo + "h", h, 72, BITPIX[code] if bitpix is None else bitpix)           # bitpix
    struct.pack_into(bo + "8f", h, 76, *([1.0] * 8))                                        # pixdim
    struct.pack_into(bo + "f", h, 108, vox_offset)                                          # vox_offset
    struct.pack_into(bo + "f", h, 112, slope)                                               # scl_slope
    struct.pack_into(bo + "f", h, 116, inter)                                               # scl_inter
    h[344:348] = magic                                                                      # magic
    data = raw.astype(raw.dtype.newbyteorder(bo)).tobytes(order="F")
    if truncate:
        data = data[:-truncate]
    return bytes(h) + data


def parse_nifti(buf):
    """{'sizeof_hdr', 'dim', 'datatype', 'bitpix', 'pixdim', 'vox_offset', 'scl_slope', 'scl_inter', 'magic', 'sform_code', 'srow', 'data'}
    of little-endian single-file NIfTI-1 bytes; data as an (x, y, z) array."""
    h = {"sizeof_hdr": struct.unpack_from("<i", buf, 0)[0], "dim": struct.unpack_from("<8h", buf, 40),
         "datatype": struct.unpack_from("<h", buf, 70)[0], "bitpix": struct.unpack_from("<h", buf, 72)[0],
         "pixdim": struct.unpack_from("<8f", buf, 76), "vox_offset": struct.unpack_from("<f", buf, 108)[0],
         "scl_slope": struct.unpack_from("<f", buf, 112)[0], "scl_inter": struct.unpack_from("<f", buf, 116)[0],
         "magic": bytes(buf[344:348]), "sform_code": struct.unpack_from("<h", buf, 254)[0],
         "srow": np.asarray(struct.unpack_from("<12f", buf, 280)).reshape(3, 4)}
    shape = h["dim"][1:1 + h["dim"][0]]
    n = int(np.prod(shape))
    h["data"] = np.frombuffer(buf, dtype="<" + NP_OF_CODE[h["datatype"]], count=n, offset=int(h["vox_offset"])).reshape(shape, order="F")
    return h


def read_nifti_file(path):
    path = str(path)
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        return parse_nifti(f.read())
