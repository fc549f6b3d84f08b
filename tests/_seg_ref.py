"""Helpers of the DICOM SEG tests: the numpy restatement of the `mmnn_unpack_frames` contract (include/mmnn_sts.h), the restatement of
the placement of frames against a scan (on the scan's grid, or on a stack of their own with one empty slice on either side), and a
struct-based packer of Segmentation objects at the published element layout (through tests/_dicom_ref.py; it shares no code with
synth_dicom).  Shares no code with mmnn_sts_amd."""
import numpy as np

from tests import _dicom_ref as D
from tests._rtstruct_ref import sequence

SEG = "1.2.840.10008.5.1.4.1.1.66.4"


# ---- the restatement of the kernel ---------------------------------------------------------------------------------------------------
def unpack_ref(bits, n_frames, refs, slice_first, shape, one=1):
    """(x, y, z) uint8: `np.unpackbits(..., bitorder="little")` over the whole stream, cut into n_frames frames of y rows of x pixels;
    slice k is the OR of the frames refs[slice_first[k]:slice_first[k + 1]] with 0 <= f < n_frames, times `one`.  A slice range that
    is not 0 <= first <= last <= len(refs) is ignored as a whole."""
    x, y, z = shape
    stream = np.unpackbits(np.frombuffer(bytes(bits), dtype=np.uint8), bitorder="little")
    assert stream.size >= n_frames * x * y, "the stream is shorter than its frames"
    frames = stream[:n_frames * x * y].reshape(n_frames, y, x)
    refs = np.asarray(refs, dtype=np.int64).reshape(-1)
    out = np.zeros(shape, dtype=np.uint8)
    for k in range(z):
        lo, hi = int(slice_first[k]), int(slice_first[k + 1])
        if not 0 <= lo <= hi <= len(refs):
            continue
        for f in refs[lo:hi]:
            if 0 <= f < n_frames:
                out[:, :, k] |= frames[f].T
    return out * np.uint8(one)


def pack_frames(frames, pad_ones=True, even=True):
    """The PixelData bytes of 2-D (rows, columns) 0 / 1 arrays: every frame row-major, bit after bit, least significant bit of a byte
    first, the frames back to back without byte alignment; the pad bits behind the last frame are all set when `pad_ones`, and the
    value is padded to even length with 0xFF."""
    flat = np.concatenate([np.asarray(f, dtype=np.uint8).reshape(-1) for f in frames]) if len(frames) else np.zeros(0, dtype=np.uint8)
    data = bytearray((flat.size + 7) // 8)
    for b in np.flatnonzero(flat):
        data[b >> 3] |= 1 << (b & 7)
    if pad_ones:
        for b in range(flat.size, 8 * len(data)):
            data[b >> 3] |= 1 << (b & 7)
    if even and len(data) % 2:
        data.append(0xFF)
    return bytes(data)


# ---- the restatement of the placement -------------------------------------------------------------------------------------------------
def scan_index(lps, affine):
    """LPS millimetres -> continuous voxel index of a scan with the RAS voxel-index -> mm matrix `affine`, term by term."""
    m = np.linalg.inv(np.asarray(affine, dtype=np.float64))
    rx, ry, rz = -float(lps[0]), -float(lps[1]), float(lps[2])
    return np.array([m[r][0] * rx + m[r][1] * ry + m[r][2] * rz + m[r][3] for r in range(3)])


def on_scan_ref(positions, orientation, spacing, shape, affine, tolerance=1e-3):
    """Slice index per frame when the corners (0,0), (x-1,0), (0,y-1) of every frame map to within `tolerance` of (0,0,k), (x-1,0,k),
    (0,y-1,k) of the scan for one integer k per frame, else None.  `spacing`: PixelSpacing (between rows, between columns)."""
    x, y, _ = shape
    r, c = np.asarray(orientation[:3], dtype=np.float64), np.asarray(orientation[3:], dtype=np.float64)
    ks = []
    for p in np.asarray(positions, dtype=np.float64):
        a, b, d = scan_index(p, affine), scan_index(p + r * spacing[1] * (x - 1), affine), scan_index(p + c * spacing[0] * (y - 1), affine)
        k = float(np.rint(a[2]))
        err = max(np.abs(a - (0, 0, k)).max(), np.abs(b - (x - 1, 0, k)).max(), np.abs(d - (0, y - 1, k)).max())
        if err > tolerance:
            return None
        ks.append(int(k))
    return ks


def own_grid_ref(positions, orientation, spacing, step, rows, columns):
    """(shape, RAS affine, slice per frame) of the stack the frames form: slice 1 is the lowest frame along the normal, slice 0 and
    the last one are empty.  The slice vector runs from the lowest to the highest position, divided by the number of steps between."""
    p = np.asarray(positions, dtype=np.float64)
    r, c = np.asarray(orientation[:3], dtype=np.float64), np.asarray(orientation[3:], dtype=np.float64)
    n = np.cross(r, c)
    along = p @ n
    idx = np.rint((along - along.min()) / step).astype(int)
    top = int(idx.max())
    lo, hi = p[int(np.argmin(along))], p[int(np.argmax(along))]
    v = (hi - lo) / top if top else n * step
    lps = np.eye(4)
    lps[:3, 0], lps[:3, 1], lps[:3, 2], lps[:3, 3] = r * spacing[1], c * spacing[0], v, lo - v
    return (columns, rows, top + 3), np.diag([-1.0, -1.0, 1.0, 1.0]) @ lps, (idx + 1).tolist()


def arrays(slices, frames, z):
    """refs / slice_first from the slice of every listed frame (the file's order within a slice)."""
    order = sorted(range(len(slices)), key=lambda i: slices[i])
    refs = np.asarray([frames[i] for i in order], dtype=np.int32)
    ordered = [slices[i] for i in order]
    return refs, np.asarray([sum(1 for s in ordered if s < k) for k in range(z + 1)], dtype=np.int32)


# ---- packing files -------------------------------------------------------------------------------------------------------------------
def number(v):
    return repr(float(v))


def seg_file(rows, columns, segments, frames, pixels, orientation=(1, 0, 0, 0, 1, 0), spacing=(1.0, 1.0), thickness=2.0, between=None,
             where="shared", explicit=True, undefined=False, sop_class=SEG, kind="BINARY", bits=1, syntax=None, declared_frames=None,
             pixel_length=None, extra=b""):
    """`segments`: [(SegmentNumber, SegmentLabel)]; `frames`: [(ReferencedSegmentNumber or None, position or None)] in PixelData order
    (None leaves the functional group out of that frame's item); `where`: 'shared' or 'frame' -- which functional group sequence holds
    orientation and pixel measures -- or None for no orientation anywhere (pixel measures stay shared).  A sequence the reader has no
    use for (DerivationImageSequence) sits in front of every frame's groups."""
    e = lambda g, n, vr, v: D.el(g, n, vr, v, explicit)
    seq = lambda g, n, items: sequence(g, n, items, explicit, undefined)
    measures = e(0x0018, 0x0050, "DS", number(thickness)) if thickness is not None else b""
    if between is not None:
        measures += e(0x0018, 0x0088, "DS", number(between))
    if spacing is not None:
        measures += e(0x0028, 0x0030, "DS", "\\".join(number(v) for v in spacing))
    plane = seq(0x0020, 0x9116, [e(0x0020, 0x0037, "DS", "\\".join(number(v) for v in orientation))]) if where else b""
    measured = seq(0x0028, 0x9110, [measures])
    per_frame = []
    for n, position in frames:
        item = seq(0x0008, 0x9124, [e(0x0008, 0x1155, "UI", "1.2.3.4")])
        if position is not None:
            item += seq(0x0020, 0x9113, [e(0x0020, 0x0032, "DS", "\\".join(number(v) for v in position))])
        if where == "frame":
            item += plane + measured
        if n is not None:
            item += seq(0x0062, 0x000A, [e(0x0062, 0x000B, "US", D.us(n))])
        per_frame.append(item)
    shared = (plane if where == "shared" else b"") + (measured if where != "frame" else b"")
    described = [e(0x0062, 0x0004, "US", D.us(n)) + e(0x0062, 0x0005, "LO", label) for n, label in segments]
    body = (e(0x0062, 0x0001, "CS", kind) + seq(0x0062, 0x0002, described) + seq(0x5200, 0x9229, [shared]) + seq(0x5200, 0x9230, per_frame))
    head = {(0x0008, 0x0016): ("UI", sop_class), (0x0008, 0x0060): ("CS", "SEG"), (0x0028, 0x0002): ("US", D.us(1)),
            (0x0028, 0x0008): ("IS", str(len(frames) if declared_frames is None else declared_frames)), (0x0028, 0x0010): ("US", D.us(rows)),
            (0x0028, 0x0011): ("US", D.us(columns)), (0x0028, 0x0100): ("US", D.us(bits)), (0x0028, 0x0101): ("US", D.us(bits)),
            (0x0028, 0x0102): ("US", D.us(bits - 1)), (0x0028, 0x0103): ("US", D.us(0))}
    return D.part10(head, pixels, explicit, syntax, extra=body + extra, pixel_length=pixel_length, pixel_vr="OB")


# the RAS affine of a scan whose LPS millimetres are (i, j, 2 k): voxel index = (x_lps, y_lps, z / 2)
LPS_AFFINE = np.diag([-1.0, -1.0, 2.0, 1.0])
