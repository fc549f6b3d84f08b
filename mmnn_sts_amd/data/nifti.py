"""A minimal NIfTI-1 single-file reader and writer (numpy, gzip and struct only; nibabel is not a dependency).

Pinned to the published NIfTI-1 header layout (348 bytes): `sizeof_hdr`@0 (int32, = 348 in the file's byte order), `dim`@40 (8 x int16),
`datatype`@70, `bitpix`@72 (int16), `pixdim`@76 (8 x float32), `vox_offset`@108, `scl_slope`@112, `scl_inter`@116 (float32),
`magic`@344 (`n+1\\0`); the geometry: `qform_code`@252, `sform_code`@254 (int16), `quatern_b/c/d`@256, `qoffset_x/y/z`@268,
`srow_x/y/z`@280/296/312 (4 x float32 each).  Parity with nibabel is unpinned (it is not installed where this was written).

`read(path)` returns the voxels IN THEIR ON-DISK TYPE, native byte order, as a numpy array of shape `dim[1..ndim]` whose memory is the
file's (x fastest = Fortran order) -- what the device ingest (`mmnn_sts_amd.data.ingest`) uploads -- together with scl_slope / scl_inter.
`NiftiImage.get_fdata()` is the float64 array nibabel's `get_fdata()` hands upstream: `raw * slope + inter`, unscaled when the slope is
0, NaN or infinite.  The writer emits what upstream's inference writes (`nib.Nifti1Image(array, affine=np.eye(4))`): float32 / int16 /
uint8, identity affine, `vox_offset` 352.  RGB / complex types and header pairs (`.hdr` / `.img`, magic `ni1`) are refused.

`NiftiImage.affine` is the 4x4 float64 voxel-index -> millimetre matrix by the published rules, in nibabel's order of preference: the
sform rows when `sform_code > 0`; else, when `qform_code > 0`, the quaternion's rotation (a = sqrt(max(0, 1 - b^2 - c^2 - d^2))) with its
columns scaled by `pixdim[1..3]`, the third also by qfac = `pixdim[0]` (0 read as +1), and the `qoffset`s as translation; else None,
"no geometry".  `write(..., affine=A)` stores A as the sform (float32, `sform_code` 2).  `index_map(scan, mask)` is the matrix the
device resample of a mask drawn on another grid takes (`mmnn_sts_amd.data.ingest.resample_mask`).
"""
import gzip
import math
import os
import struct
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..exceptions.exceptions import ConfigurationError

# datatype code -> (numpy dtype character, bitpix)
DTYPES = {2: ("u1", 8), 4: ("i2", 16), 8: ("i4", 32), 16: ("f4", 32), 64: ("f8", 64), 256: ("i1", 8), 512: ("u2", 16), 768: ("u4", 32)}
_REFUSED = {32: "complex64", 128: "RGB24", 1792: "complex128", 2048: "complex256", 2304: "RGBA32", 1536: "float128", 1024: "int64",
            1280: "uint64", 1: "binary"}
_WRITE_CODES = {np.dtype("float32"): 16, np.dtype("int16"): 4, np.dtype("uint8"): 2}
HEADER_BYTES = 348
VOX_OFFSET = 352


@dataclass
class NiftiImage:
    raw: np.ndarray          # on-disk type, native byte order, shape dim[1..ndim] (trailing extents of 1 beyond the third dropped), x fastest
    datatype: int            # NIfTI datatype code
    slope: float             # scl_slope as stored (float32 widened)
    inter: float             # scl_inter as stored
    path: str = ""
    affine: Optional[np.ndarray] = None      # 4x4 float64 voxel index -> mm (sform, else qform); None: the file has no geometry

    @property
    def shape(self):
        return self.raw.shape

    def scaling(self):
        """(slope, inter) to apply, or None for "no scaling": nibabel ignores both when the slope is 0, NaN or infinite, and reads
        a non-finite inter as 0."""
        if self.slope == 0.0 or not math.isfinite(self.slope):
            return None
        return float(self.slope), (float(self.inter) if math.isfinite(self.inter) else 0.0)

    def get_fdata(self) -> np.ndarray:
        s = self.scaling()
        a = self.raw.astype(np.float64)
        if s is None or s == (1.0, 0.0):
            return a
        return a * s[0] + s[1]


def _open_bytes(path: str) -> bytes:
    if path.endswith(".gz"):
        with gzip.open(path, "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


def _affine_of(buf, bo: str) -> Optional[np.ndarray]:
    """The header's geometry: sform when its code is set, else qform, else None."""
    qform_code, sform_code = struct.unpack_from(bo + "2h", buf, 252)
    a = np.eye(4, dtype=np.float64)
    if sform_code > 0:
        a[:3, :] = np.asarray(struct.unpack_from(bo + "12f", buf, 280), dtype=np.float64).reshape(3, 4)
        return a
    if qform_code > 0:
        b, c, d = (float(v) for v in struct.unpack_from(bo + "3f", buf, 256))
        pixdim = [float(v) for v in struct.unpack_from(bo + "4f", buf, 76)]
        qa = math.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
        rot = np.array([[qa * qa + b * b - c * c - d * d, 2.0 * (b * c - qa * d), 2.0 * (b * d + qa * c)],
                        [2.0 * (b * c + qa * d), qa * qa + c * c - b * b - d * d, 2.0 * (c * d - qa * b)],
                        [2.0 * (b * d - qa * c), 2.0 * (c * d + qa * b), qa * qa + d * d - b * b - c * c]])
        qfac = -1.0 if pixdim[0] < 0.0 else 1.0
        a[:3, :3] = rot * np.array([pixdim[1], pixdim[2], pixdim[3] * qfac])
        a[:3, 3] = struct.unpack_from(bo + "3f", buf, 268)
        return a
    return None


def _byte_order(buf, path: str) -> str:
    if len(buf) < HEADER_BYTES:
        raise ConfigurationError(f"{path}: {len(buf)} bytes, shorter than a NIfTI-1 header")
    if struct.unpack_from("<i", buf, 0)[0] == HEADER_BYTES:
        return "<"
    if struct.unpack_from(">i", buf, 0)[0] == HEADER_BYTES:
        return ">"
    raise ConfigurationError(f"{path}: sizeof_hdr is not 348 in either byte order (not a NIfTI-1 file)")


def read_geometry(path: str):
    """(extents dim[1..ndim] with trailing 1s beyond the third dropped, affine or None) from the header alone: the voxels are not read
    (a .gz is inflated only as far as the header)."""
    path = str(path)
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        buf = f.read(HEADER_BYTES)
    bo = _byte_order(buf, path)
    dim = struct.unpack_from(bo + "8h", buf, 40)
    shape = [int(d) for d in dim[1:1 + max(0, min(7, dim[0]))]]
    while len(shape) > 3 and shape[-1] == 1:
        shape.pop()
    return tuple(shape), _affine_of(buf, bo)


def index_map(scan, mask) -> np.ndarray:
    """The (3, 4) float64 matrix that takes a scan voxel index (i, j, k, 1) to a continuous index into the mask's grid:
    inv(mask.affine) @ scan.affine.  `scan`, `mask`: anything with `.affine` (and `.path`, named in the refusal)."""
    mats = []
    for what, v in (("scan", scan), ("mask", mask)):
        a = getattr(v, "affine", None)
        name = getattr(v, "path", "") or f"the {what}"
        if a is None:
            raise ConfigurationError(f"{name}: no qform/sform in the header, so the mask cannot be resampled into the scan's grid")
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (4, 4) or not np.isfinite(a).all():
            raise ConfigurationError(f"{name}: the affine is not a finite 4x4 matrix")
        mats.append((name, a))
    (_, sa), (mname, ma) = mats
    scale = np.abs(ma[:3, :3]).max()
    if scale == 0.0 or abs(np.linalg.det(ma[:3, :3] / scale)) < 1e-12 or ma[3, 3] == 0.0:
        raise ConfigurationError(f"{mname}: the affine is singular, so the mask cannot be resampled into the scan's grid")
    t = np.linalg.inv(ma) @ sa
    return np.ascontiguousarray(t[:3, :])


def read(path: str) -> NiftiImage:
    path = str(path)
    buf = _open_bytes(path)
    bo = _byte_order(buf, path)
    magic = buf[344:348]
    if magic != b"n+1\0":
        what = "a header pair (.hdr/.img)" if magic[:3] == b"ni1" else f"magic {magic!r}"
        raise ConfigurationError(f"{path}: {what} is not supported, only single-file NIfTI-1 (magic 'n+1')")
    dim = struct.unpack_from(bo + "8h", buf, 40)
    datatype, bitpix = struct.unpack_from(bo + "2h", buf, 70)
    vox_offset, slope, inter = struct.unpack_from(bo + "3f", buf, 108)
    if datatype not in DTYPES:
        name = _REFUSED.get(datatype, "unknown")
        raise ConfigurationError(f"{path}: datatype code {datatype} ({name}) is not supported (supported: {sorted(DTYPES)})")
    ch, bits = DTYPES[datatype]
    if bitpix != bits:
        raise ConfigurationError(f"{path}: bitpix {bitpix} does not match datatype code {datatype} ({bits} bits)")
    ndim = dim[0]
    if not 1 <= ndim <= 7:
        raise ConfigurationError(f"{path}: dim[0] = {ndim}")
    shape = [int(d) for d in dim[1:1 + ndim]]
    if any(d < 1 for d in shape):
        raise ConfigurationError(f"{path}: non-positive extent in dim {shape}")
    while len(shape) > 3 and shape[-1] == 1:       # (x, y, z, 1): a volume
        shape.pop()
    off = int(vox_offset)
    if off < VOX_OFFSET:
        raise ConfigurationError(f"{path}: vox_offset {vox_offset} inside the header")
    count = int(np.prod(shape, dtype=np.int64))
    nbytes = count * (bits // 8)
    if len(buf) < off + nbytes:
        raise ConfigurationError(f"{path}: truncated: {len(buf) - off} bytes of voxel data, {nbytes} expected for {shape} of type {datatype}")
    a = np.frombuffer(buf, dtype=np.dtype(bo + ch), count=count, offset=off)
    a = a.astype(a.dtype.newbyteorder("="), copy=True)       # the swap of a foreign byte order happens here, on the host
    return NiftiImage(a.reshape(shape, order="F"), int(datatype), float(slope), float(inter), path, _affine_of(buf, bo))


def header_bytes(shape, datatype: int, slope: float = 1.0, inter: float = 0.0, byteorder: str = "<", affine=None) -> bytes:
    """A 348-byte NIfTI-1 header + 4 bytes of (empty) extension flag for a volume of `shape`: `vox_offset` 352; the sform rows are
    `affine`'s (4x4 or 3x4, stored as float32), the identity when it is None."""
    if datatype not in DTYPES:
        raise ConfigurationError(f"datatype code {datatype} is not supported")
    shape = tuple(int(s) for s in shape)
    if not 1 <= len(shape) <= 7:
        raise ConfigurationError(f"cannot write an array of {len(shape)} dimensions")
    h = bytearray(VOX_OFFSET)
    bo = byteorder
    struct.pack_into(bo + "i", h, 0, HEADER_BYTES)
    struct.pack_into(bo + "8h", h, 40, len(shape), *shape, *([1] * (7 - len(shape))))
    struct.pack_into(bo + "2h", h, 70, datatype, DTYPES[datatype][1])
    struct.pack_into(bo + "8f", h, 76, 1.0, *([1.0] * len(shape)), *([1.0] * (7 - len(shape))))
    struct.pack_into(bo + "3f", h, 108, float(VOX_OFFSET), slope, inter)
    struct.pack_into(bo + "b", h, 123, 2)                       # xyzt_units: millimetres
    struct.pack_into(bo + "2h", h, 252, 0, 2)                   # qform_code 0, sform_code 2 (aligned)
    struct.pack_into(bo + "4f", h, 280, 1.0, 0.0, 0.0, 0.0)     # srow_x
    struct.pack_into(bo + "4f", h, 296, 0.0, 1.0, 0.0, 0.0)     # srow_y
    struct.pack_into(bo + "4f", h, 312, 0.0, 0.0, 1.0, 0.0)     # srow_z
    if affine is not None:
        a = np.asarray(affine, dtype=np.float64)
        if a.shape not in ((4, 4), (3, 4)) or not np.isfinite(a).all():
            raise ConfigurationError(f"affine must be a finite 4x4 (or 3x4) matrix, got shape {a.shape}")
        struct.pack_into(bo + "12f", h, 280, *a[:3, :].reshape(-1))
    h[344:348] = b"n+1\0"
    return bytes(h)


def write(path: str, array, slope: float = 1.0, inter: float = 0.0, affine=None) -> str:
    """Write `array` (float32, int16 or uint8; any memory layout) as a single-file NIfTI-1 volume with `affine` as its sform (the
    identity when None); gzip when the name ends in .gz."""
    path = str(path)
    a = np.asarray(array)
    if a.dtype not in _WRITE_CODES:
        raise ConfigurationError(f"cannot write dtype {a.dtype}: float32, int16 and uint8 are supported")
    data = header_bytes(a.shape, _WRITE_CODES[a.dtype], slope, inter, affine=affine) + a.astype(a.dtype.newbyteorder("<")).tobytes(order="F")
    if path.endswith(".gz"):
        with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, compresslevel=1, mtime=0) as f:
            f.write(data)
    else:
        with open(path, "wb") as f:
            f.write(data)
    return path
