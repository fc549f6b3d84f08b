"""Raw scans -> the device batch: binding of `mmnn_ingest_volume` (csrc/ingest.hip) and the collate function built on it.

What upstream's NIfTI datasets do per patient and modality in `__getitem__` (data/ImageDatasets.py:431-470, :599-637: image * mask,
every all-zero slice dropped along each axis, Resize((64,64,64)), T1 / T2 stacked along the channel axis) runs here on the device, from
the file's voxels in their on-disk type.  The host only uploads bytes (pinned, non-blocking) and enqueues; it never waits.

    upload(volume, device)                          host volume (NiftiImage, DicomSeries or ndarray) -> DeviceVolume
    stage_mask(scan, mask, device)                  host mask of any source -> DeviceVolume, or Staged{Contours,Frames} that wait for their kernel
    decode_series(series, device)                   a sorted DICOM series -> DeviceVolume: the slices' bytes decoded on device (mmnn_decode_slices)
                                                    (an RLE Lossless series: its fragments expanded first, mmnn_rle_expand; a JPEG
                                                    Lossless series: Huffman-decoded and predicted first, mmnn_jpegll_decode)
    rasterize_contours(contours, scan, device)      the contours of an RTSTRUCT ROI -> uint8 0 / 1 on the scan's grid (mmnn_rasterize_contours)
    unpack_frames(frames, scan, device)             the frames of a DICOM SEG segment -> uint8 0 / 1 on the scan's grid, or 0 / 255 on the
                                                    segmentation's own (mmnn_unpack_frames)
    resample_mask(mask, scan_shape, index_map)      a mask drawn on another grid -> uint8 bytes on the scan's grid (mmnn_resample_mask)
    prepare_pair(scan, mask, device)                upload, rasterise / unpack / resample the mask: the pair on one grid, on the device
    ingest_volume(scan, mask, out_plane, extents)   one volume -> one S^3 channel plane, S = the plane's extent (the mask is resampled first when its grid differs)
    collate_volumes(patients, device, size=64)      [[(scan, mask) per modality] per patient] -> (N, C, S,S,S) fp32, (N, C, 3) int32
    ingest_patients(patients, device, into)         the uploads and launches of collate_volumes, into destinations the caller names
    IngestCollate(device, size=64, cache=None)      the DataLoader collate_fn of the NIfTI datasets; `cache`: a VolumeCache (data/cache.py)
                                                    that keeps every ingested patient on the device and assembles the batches from it
    mask_margin(mask, spacing, radius_mm, mode)     a mask on the scan's grid -> uint8 0 / 1: the mask widened by a margin in mm ('dilate'), or
                                                    the shell of that width around it ('shell') (mmnn_mask_margin)
    maps_to_scan(maps, scan_shape, ingest_workspace)   the way back: S^3 model-space maps -> fp32 volumes on the scan's grid (mmnn_maps_to_scan_sized)

The output extent S is 64 (`SIZE`, upstream's Resize target) unless a caller chooses another one in 1..128 (`MAX_SIZE`): `ingest_volume`
reads it off the plane it is given, `maps_to_scan` off the maps, the collate functions take `size=`.

A mask on another grid (a T2 contour used on the T1 scan, a resliced export, a mask cropped to the tumour's bounding box) is what
upstream's DICOM datasets pass through `sitk.Resample(mask, image)` and `> 128` (data/ImageDatasets.py:145-152, :246-257); here the
host forms one 3x4 matrix from the two headers (`nifti.index_map`) and the device does the rest.  `Data: mask_resample` selects when:
'auto' (only when the extents differ), 'geometry' (also when equal extents sit elsewhere in space), 'never'.

A DICOM series (`dicom.read_series`) takes one more step in front: its slices' PixelData bytes are uploaded as the files hold them and
`mmnn_decode_slices` unpacks the stored bits, extends the sign and, where the slices differ in RescaleSlope / RescaleIntercept, rescales
per slice.  An RLE Lossless series uploads its fragments as the files hold them, `mmnn_rle_expand` turns them into the bytes the uncompressed
series would hold, and `mmnn_decode_slices` follows unchanged; the z status words are read back once per series, and a slice whose
segment ended early is refused with its file named.  A JPEG Lossless series goes the same way through `mmnn_jpegll_decode`, with a
record per frame (where its entropy-coded data lies, its precision and its Huffman table) in place of the segment table.  A DICOM (scan, mask) pair always passes through `resample_mask` -- upstream always runs `sitk.Resample(mask, image)` and
`mask > 128` on that path -- with the identity map when the two series share one grid, and its default threshold is 128.

A mask that is an RT Structure Set (`rtstruct.read` -> `ContourSet`) beside a DICOM scan is born on the scan's grid: the host maps the
contour points into the scan's voxel index space (`rtstruct.to_scan_index`), `mmnn_rasterize_contours` fills them by the even-odd rule
into 0 / 1 bytes, and the pair takes the voxelwise path -- no resample, no threshold.

A mask that is a DICOM Segmentation object (`seg.read` -> `FrameSet`) beside a DICOM scan: the host places the frames of the selected
segment against the scan (`seg.to_scan`) and `mmnn_unpack_frames` unpacks the bit-packed PixelData, uploaded as the file holds it.
Frames on the scan's slice planes are written as 0 / 1 straight onto the scan's grid and take the voxelwise path like an RTSTRUCT
mask; a segmentation on a grid of its own is unpacked as 0 / 255 onto its own stack and then takes the path of a DICOM mask series
(`resample_mask` by `nifti.index_map`, binarised at `mask_threshold` or 128).
"""
import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from ..exceptions.exceptions import ConfigurationError
from . import nifti, rtstruct, seg
from .dicom import JPEGLL, RLE, DicomSeries
from .nifti import NiftiImage
from .rtstruct import ContourSet
from .seg import FrameSet

SIZE = 64                                    # MMNN_INGEST_SIZE: the default output extent per axis
MAX_SIZE = 128                               # MMNN_INGEST_MAX_SIZE: the largest one
MASK_RESAMPLE_MODES = ("auto", "geometry", "never")
GEOMETRY_TOLERANCE = 1e-3                    # voxels: 'geometry' resamples when a corner of the scan grid maps further from itself
NIFTI_MASK_THRESHOLD, DICOM_MASK_THRESHOLD = 0.5, 128.0          # defaults of `Data: mask_threshold` (upstream: `mask > 128`)
IDENTITY_MAP = np.eye(4, dtype=np.float64)[:3]
TYPE_CODES = {np.dtype("uint8"): 2, np.dtype("int16"): 4, np.dtype("int32"): 8, np.dtype("float32"): 16, np.dtype("float64"): 64,
              np.dtype("int8"): 256, np.dtype("uint16"): 512, np.dtype("uint32"): 768}


@dataclass
class DeviceVolume:
    """A scan's voxels on the device as the file holds them: `data` is a flat uint8 tensor of x*y*z elements of NIfTI type `datatype`,
    x fastest.  `affine`: the file's voxel index -> mm matrix when it has one.  `from_dicom`: decoded from a DICOM series (its mask
    is always resampled, and binarised at 128 by default)."""
    data: torch.Tensor
    shape: Tuple[int, int, int]
    datatype: int
    slope: float = 1.0
    inter: float = 0.0
    affine: Optional[np.ndarray] = None
    from_dicom: bool = False


@dataclass
class KeptVolume:
    """What `keep_workspaces` retains of one ingested volume: the ingest's workspace (its kept-index lists and extents, which
    `maps_to_scan` reads), the scan's extents and its affine (None: the file has no geometry)."""
    workspace: torch.Tensor
    shape: Tuple[int, int, int]
    affine: Optional[np.ndarray] = None


@dataclass
class RawPatient:
    """What an image dataset's `__getitem__` yields in place of a float volume: per modality the (scan, mask) pair, still raw (two
    NiftiImages, two DicomSeries, or a DicomSeries and the ContourSet of its RTSTRUCT mask or the FrameSet of its SEG mask)."""
    uid: int
    volumes: List[Tuple[object, object]]


def _host_bytes(raw: np.ndarray) -> np.ndarray:
    """The volume's bytes with x fastest, without a copy when the array already is x-fastest (as the reader returns it)."""
    if raw.ndim != 3:
        raise ValueError(f"ingest: a volume has three axes, got an array of shape {raw.shape}")
    if raw.dtype not in TYPE_CODES:
        raise ValueError(f"ingest: dtype {raw.dtype} has no supported NIfTI type code ({sorted(str(k) for k in TYPE_CODES)})")
    return np.ascontiguousarray(raw.T).reshape(-1).view(np.uint8)


def upload(volume, device, slope: float = 1.0, inter: float = 0.0) -> DeviceVolume:
    """Host -> device, in the on-disk type.  `volume`: a NiftiImage (its slope / inter are used), a DicomSeries (`decode_series`) or
    an (x, y, z) ndarray."""
    if isinstance(volume, DeviceVolume):
        return volume
    if isinstance(volume, DicomSeries):
        return decode_series(volume, device)
    if isinstance(volume, FrameSet):
        raise ValueError(f"ingest: a SEG mask ({volume.path}) is placed against its scan: upload it with stage_frames(frames, scan, device)")
    affine = None
    if isinstance(volume, NiftiImage):
        raw, slope, inter, affine = volume.raw, volume.slope, volume.inter, volume.affine
    else:
        raw = np.asarray(volume)
    if not raw.dtype.isnative:
        raw = raw.astype(raw.dtype.newbyteorder("="))
    host = torch.from_numpy(_host_bytes(raw)).pin_memory()
    return DeviceVolume(host.to(device, non_blocking=True), tuple(int(s) for s in raw.shape), TYPE_CODES[raw.dtype], float(slope), float(inter), affine)


def _integer_code(bits_allocated: int, signed: bool) -> int:
    return TYPE_CODES[np.dtype(f"{'i' if signed else 'u'}{bits_allocated // 8}")]


def decode_series(series: DicomSeries, device) -> DeviceVolume:
    """A sorted DICOM series -> its voxels on the device, (Columns, Rows, slices) with the column fastest.  One pinned staging buffer
    (the per-slice scale table when it is needed, then the slices' bytes in sorted order), one non-blocking copy and one
    `mmnn_decode_slices` on the current stream; the host copies bytes and touches no voxel value.  When every slice carries the same
    RescaleSlope / RescaleIntercept and the ingest's descriptor holds that pair exactly (it carries float32, as a NIfTI header does),
    the volume keeps the integer type of (BitsAllocated, PixelRepresentation) and the pair goes into `slope` / `inter`, which the
    ingest applies in fp64 like a NIfTI scl_slope; otherwise the kernel rescales per slice and the volume is float64, slope 1, inter 0.
    An RLE Lossless series (`series.encoding == 'rle'`) stages its segment table and its fragments in place of the slices' bytes,
    each fragment on a 16-byte boundary, and `mmnn_rle_expand` runs in front of `mmnn_decode_slices`; the z status words are then read
    back -- the one wait of this path -- and a slice whose segment ended before its plane was full raises ConfigurationError.  A JPEG
    Lossless series (`'jpeg-lossless'`) does the same with `mmnn_jpegll_decode` and a frame record per slice."""
    if not series.frames:
        raise ValueError(f"decode_series: {series.path} was read with header_only: it holds no voxel bytes")
    device = torch.device(device)
    x, y, z = (int(v) for v in series.shape)
    if series.encoding == RLE:
        return _decode_rle_series(series, device, x, y, z)
    if series.encoding == JPEGLL:
        return _decode_jpegll_series(series, device, x, y, z)
    frame_bytes = x * y * (series.bits_allocated // 8)
    if len(series.frames) != z or any(f.dtype != np.uint8 or f.size != frame_bytes for f in series.frames):
        raise ValueError(f"decode_series: {series.path}: {z} slices of {frame_bytes} bytes expected")
    scale = series.uniform_scale()
    integer = scale is not None and all(float(np.float32(v)) == v for v in scale)
    table_bytes = 0 if integer else z * 16
    stage = torch.empty(table_bytes + z * frame_bytes, dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    if not integer:
        host[:z * 16].view(np.float64)[:] = np.asarray([v for pair in zip(series.slopes, series.inters) for v in pair], dtype=np.float64)
    for k, frame in enumerate(series.frames):
        host[table_bytes + k * frame_bytes:table_bytes + (k + 1) * frame_bytes] = frame
    code = _integer_code(series.bits_allocated, series.signed) if integer else TYPE_CODES[np.dtype("float64")]
    desc = _lib.DecodeSlicesDesc(x, y, z, series.bits_allocated, series.bits_stored, series.high_bit, int(series.signed), code)
    staged = stage.to(device, non_blocking=True)
    out = torch.empty(x * y * z * (series.bits_allocated // 8 if integer else 8), dtype=torch.uint8, device=device)
    _lib.enqueue("mmnn_decode_slices", ctypes.byref(desc), staged.data_ptr() + table_bytes, None if integer else staged.data_ptr(), out.data_ptr(),
                 device=device)
    slope, inter = scale if integer else (1.0, 0.0)
    return DeviceVolume(out, (x, y, z), code, float(slope), float(inter), series.affine, from_dicom=True)


@dataclass
class _StagedFragments:
    """What the compressed series share in front of their kernel.  The pinned buffer `stage` (`host`: its numpy view): the scale table
    (when needed), the per-frame records at `at_records`, then the payload at `at_payload`, i.e. the fragments in sorted order, each
    start (`starts[k]`, relative to the payload) aligned to 16 bytes and the gaps zeroed."""
    stage: torch.Tensor
    host: np.ndarray
    at_records: int
    at_payload: int
    starts: np.ndarray
    payload_bytes: int
    scale: Optional[Tuple[float, float]]
    integer: bool


def _stage_fragments(series: DicomSeries, z: int, record_bytes: int) -> _StagedFragments:
    """Stage the fragments of a compressed series; the caller fills the z records of `record_bytes` (a multiple of 8) each."""
    scale = series.uniform_scale()
    integer = scale is not None and all(float(np.float32(v)) == v for v in scale)
    at_records = 0 if integer else z * 16
    at_payload = (at_records + z * record_bytes + 15) // 16 * 16
    starts = np.zeros(z + 1, dtype=np.int64)
    np.cumsum([(f.size + 15) // 16 * 16 for f in series.frames], out=starts[1:])
    stage = torch.empty(at_payload + int(starts[-1]), dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    if not integer:
        host[:at_records].view(np.float64)[:] = np.asarray([v for pair in zip(series.slopes, series.inters) for v in pair], dtype=np.float64)
    host[at_records + z * record_bytes:at_payload] = 0
    for k, frame in enumerate(series.frames):
        at = at_payload + int(starts[k])
        host[at:at + frame.size] = frame
        host[at + frame.size:at_payload + int(starts[k + 1])] = 0
    return _StagedFragments(stage, host, at_records, at_payload, starts, int(starts[-1]), scale, integer)


def _decode_staged(series: DicomSeries, device, shape, s: _StagedFragments, call: str, workspace: str, desc_type, fault: str) -> DeviceVolume:
    """The staged fragments, their records filled, through `call` (`mmnn_rle_expand` or `mmnn_jpegll_decode`, with the bytes that
    `workspace`, its `*_workspace_bytes`, asks for) into the bytes of the uncompressed series, then `mmnn_decode_slices` and the one
    read-back of the z status words; a frame whose word is not 0 raises ConfigurationError with its file and `fault`."""
    x, y, z = shape
    staged = s.stage.to(device, non_blocking=True)
    words = torch.empty(x * y * z * (series.bits_allocated // 8), dtype=torch.uint8, device=device)
    status = torch.empty(z, dtype=torch.int32, device=device)
    ws = torch.empty(_lib.count(workspace, x, y, z, series.bits_allocated), dtype=torch.uint8, device=device)
    desc = desc_type(x, y, z, series.bits_allocated, s.payload_bytes)
    _lib.enqueue(call, ctypes.byref(desc), staged.data_ptr() + s.at_payload, staged.data_ptr() + s.at_records, words.data_ptr(),
                 status.data_ptr(), ws.data_ptr(), device=device)
    code = _integer_code(series.bits_allocated, series.signed) if s.integer else TYPE_CODES[np.dtype("float64")]
    desc = _lib.DecodeSlicesDesc(x, y, z, series.bits_allocated, series.bits_stored, series.high_bit, int(series.signed), code)
    out = torch.empty(x * y * z * (series.bits_allocated // 8 if s.integer else 8), dtype=torch.uint8, device=device)
    _lib.enqueue("mmnn_decode_slices", ctypes.byref(desc), words.data_ptr(), None if s.integer else staged.data_ptr(), out.data_ptr(), device=device)
    bad = np.flatnonzero(status.cpu().numpy())
    if bad.size:
        k = int(bad[0])
        name = series.files[k] if k < len(series.files) else f"{series.path}: slice {k}"
        raise ConfigurationError(f"{name}: malformed: {fault} ({bad.size} of the {z} slices of {series.path} are short)")
    slope, inter = s.scale if s.integer else (1.0, 0.0)
    return DeviceVolume(out, (x, y, z), code, float(slope), float(inter), series.affine, from_dicom=True)


def _decode_rle_series(series: DicomSeries, device, x: int, y: int, z: int) -> DeviceVolume:
    """`decode_series` of an RLE Lossless series.  The records of the pinned buffer (`_stage_fragments`): the segment table, [z][B][2]
    int64: byte offset into the payload, byte length."""
    planes = series.bits_allocated // 8
    if len(series.frames) != z or len(series.segments) != z or any(f.dtype != np.uint8 for f in series.frames) \
            or any(np.asarray(t).shape != (planes, 2) for t in series.segments):
        raise ValueError(f"decode_series: {series.path}: {z} RLE fragments with {planes} segments each expected")
    s = _stage_fragments(series, z, planes * 16)
    table = s.host[s.at_records:s.at_records + z * planes * 16].view(np.int64).reshape(z, planes, 2)
    for k, segments in enumerate(series.segments):
        table[k] = segments
        table[k, :, 0] += s.starts[k]
    return _decode_staged(series, device, (x, y, z), s, "mmnn_rle_expand", "mmnn_rle_workspace_bytes", _lib.RleDesc,
                          f"an RLE segment ends before its {x} x {y} byte plane is full")


JPEGLL_FRAME = np.dtype([("offset", "<i8"), ("length", "<i8"), ("precision", "<i4"), ("bits", "u1", 16), ("huffval", "u1", 17), ("reserved", "u1", 3)])
assert JPEGLL_FRAME.itemsize == _lib.JPEGLL_FRAME_BYTES      # mmnn_jpegll_frame


def _decode_jpegll_series(series: DicomSeries, device, x: int, y: int, z: int) -> DeviceVolume:
    """`decode_series` of a JPEG Lossless series.  The records of the pinned buffer (`_stage_fragments`): z `mmnn_jpegll_frame`s -- where the
    entropy-coded data lies in the payload, the precision and the Huffman table, as `dicom.read_file` took them from the marker segments."""
    if len(series.frames) != z or len(series.jpeg) != z or any(f.dtype != np.uint8 for f in series.frames):
        raise ValueError(f"decode_series: {series.path}: {z} JPEG fragments with their scan headers expected")
    s = _stage_fragments(series, z, JPEGLL_FRAME.itemsize)
    records = s.host[s.at_records:s.at_records + z * JPEGLL_FRAME.itemsize].view(JPEGLL_FRAME)
    records[:] = np.zeros((), dtype=JPEGLL_FRAME)
    for k, scan in enumerate(series.jpeg):
        records[k]["offset"], records[k]["length"], records[k]["precision"] = int(s.starts[k]) + scan.offset, scan.length, scan.precision
        records[k]["bits"] = scan.bits
        records[k]["huffval"][:len(scan.huffval)] = scan.huffval
    return _decode_staged(series, device, (x, y, z), s, "mmnn_jpegll_decode", "mmnn_jpegll_workspace_bytes", _lib.JpegllDesc,
                          f"the JPEG stream ends, or holds an invalid code, before its {x} x {y} samples are decoded")


def _default_device(out):                    # where a call that names no device works
    return out.device if out is not None else torch.device("cuda", torch.cuda.current_device())


@dataclass
class StagedContours:
    """The three arrays of `rtstruct.to_scan_index` in one device buffer: a contour mask between its upload and its rasterisation
    (`collate_volumes` issues every upload first).  Like `StagedFrames` it says whether it is `on_scan` and runs its kernel in `to_volume`."""
    staged: torch.Tensor
    at_records: int                          # byte offsets of the contour records and of slice_first behind the points
    at_slices: int
    n_contours: int
    n_points: int
    slices: int
    on_scan = True                           # contours are born on the scan's grid
    no_index_map = "a contour mask is rasterised onto the scan's own grid; it takes no index_map"

    def to_volume(self, scan, out: Optional[torch.Tensor] = None) -> DeviceVolume:
        x, y, z = (int(v) for v in scan.shape)
        dev = self.staged.device
        if self.slices != z:
            raise ValueError(f"rasterize_contours: slice_first has {self.slices + 1} entries, a scan of {z} slices needs {z + 1}")
        out = _lib.device_buffer(out, x * y * z, torch.uint8, dev, "rasterize_contours")
        desc = _lib.RasterizeDesc(x, y, z, self.n_contours, self.n_points)
        p = self.staged.data_ptr()
        _lib.enqueue("mmnn_rasterize_contours", ctypes.byref(desc), p, p + self.at_records, p + self.at_slices, out.data_ptr(), device=dev)
        return DeviceVolume(out.view(-1), (x, y, z), TYPE_CODES[np.dtype("uint8")], 1.0, 0.0, getattr(scan, "affine", None))


def stage_contours(contours, scan, device, roi=None) -> StagedContours:
    """Upload a contour mask for the grid of `scan` (anything with `.shape` and `.affine`): one pinned staging buffer for the three
    arrays and one non-blocking copy.  `contours`: a ContourSet (`roi` names the ROI to take; None: its only one), placed on the
    scan's grid by `rtstruct.to_scan_index`, or the (points, contours, slice_first) arrays themselves."""
    if isinstance(contours, ContourSet):
        _placed(scan, contours, named=True)
        contours = rtstruct.to_scan_index(rtstruct.select(contours, roi), scan.shape, scan.affine)
    points, records, slice_first = (np.ascontiguousarray(a, dtype=t) for a, t in zip(contours[:3], (np.float64, np.int32, np.int32)))
    if points.ndim != 2 or points.shape[1] != 2 or records.ndim != 2 or records.shape[1] != 2 or slice_first.ndim != 1 or slice_first.size < 2:
        raise ValueError(f"rasterize_contours: points (P, 2), contours (C, 2) and slice_first (z + 1,) expected, got {points.shape}, {records.shape}, {slice_first.shape}")
    at_records = points.nbytes               # (a multiple of 16: every array starts aligned to its element size)
    at_slices = at_records + records.nbytes
    stage = torch.empty(at_slices + slice_first.nbytes, dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    host[:at_records] = points.reshape(-1).view(np.uint8)
    host[at_records:at_slices] = records.reshape(-1).view(np.uint8)
    host[at_slices:] = slice_first.view(np.uint8)
    return StagedContours(stage.to(torch.device(device), non_blocking=True), at_records, at_slices, len(records), len(points), slice_first.size - 1)


def rasterize_contours(contours, scan, device=None, roi=None, out: Optional[torch.Tensor] = None) -> DeviceVolume:
    """The contours of one ROI -> uint8 0 / 1 on the grid of `scan` (anything with `.shape` and `.affine`: a DicomSeries, a
    DeviceVolume), by the even-odd rule of `mmnn_rasterize_contours`.  `contours`: what `stage_contours` takes, or its result.  One
    pinned staging buffer, one non-blocking copy and one launch on the current stream.  `device`: None is `out`'s, else the current
    one.  `out`: a contiguous uint8 CUDA tensor of x*y*z elements to write, allocated when None.  The result is a mask of type 2,
    slope 1, inter 0 with the scan's affine -- on the scan's grid by construction, so it is neither resampled nor thresholded."""
    if not isinstance(contours, StagedContours):
        contours = stage_contours(contours, scan, _default_device(out) if device is None else device, roi)
    return contours.to_volume(scan, out)


@dataclass
class StagedFrames:
    """The bit stream of a SEG file and the two arrays of `seg.to_scan` in one device buffer: a SEG mask between its upload and its
    unpacking.  `shape`, `affine`: the grid it is unpacked onto -- the scan's (`on_scan`) or the segmentation's own."""
    staged: torch.Tensor
    at_slices: int                           # byte offsets of slice_first and of the bit stream behind refs
    at_bits: int
    n_frames: int
    n_refs: int
    shape: Tuple[int, int, int]
    affine: Optional[np.ndarray]
    one: int
    on_scan: bool
    path: str = ""
    from_dicom: bool = True
    no_index_map = "a SEG mask on the scan's own grid takes no index_map"

    def to_volume(self, scan=None, out: Optional[torch.Tensor] = None) -> DeviceVolume:
        dev = self.staged.device
        x, y, z = self.shape
        out = _lib.device_buffer(out, x * y * z, torch.uint8, dev, "unpack_frames")
        desc = _lib.UnpackFramesDesc(x, y, z, self.n_frames, self.n_refs, self.one)
        p = self.staged.data_ptr()
        _lib.enqueue("mmnn_unpack_frames", ctypes.byref(desc), p + self.at_bits, p, p + self.at_slices, out.data_ptr(), device=dev)
        return DeviceVolume(out.view(-1), (x, y, z), TYPE_CODES[np.dtype("uint8")], 1.0, 0.0, self.affine, from_dicom=not self.on_scan)


def stage_frames(frames, scan, device, roi=None) -> StagedFrames:
    """Upload a SEG mask for `scan` (anything with `.shape` and `.affine`): one pinned staging buffer (refs, slice_first, then the
    PixelData bytes as the file holds them) and one non-blocking copy.  `frames`: a FrameSet (`roi` names the segment to take; None:
    its only one), placed by `seg.to_scan`, or the arrays themselves, (bits, n_frames, refs, slice_first[, one]), for the scan's grid."""
    if isinstance(frames, FrameSet):
        _placed(scan, frames, named=True)
        if frames.header_only or frames.frame is None:
            raise ValueError(f"unpack_frames: {frames.path} was read with header_only: it holds no PixelData")
        place = seg.to_scan(seg.select(frames, roi), scan.shape, scan.affine)
        bits, n_frames, refs, slice_first, one = frames.frame, frames.n_frames, place.refs, place.slice_first, place.one
        shape, affine, on_scan, path = place.shape, place.affine, place.on_scan, frames.path
    else:
        bits, n_frames, refs, slice_first, *rest = frames
        one, shape, affine, on_scan, path = (int(rest[0]) if rest else 1), tuple(int(v) for v in scan.shape), getattr(scan, "affine", None), True, ""
    bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
    refs, slice_first = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (refs, slice_first))
    need = (int(n_frames) * shape[0] * shape[1] + 7) // 8
    if slice_first.size != shape[2] + 1 or bits.size < need:
        raise ValueError(f"unpack_frames: slice_first of {shape[2] + 1} entries and {need} bytes of frames expected, got {slice_first.size} and {bits.size}")
    at_slices = refs.nbytes
    at_bits = at_slices + slice_first.nbytes
    stage = torch.empty(at_bits + need, dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    host[:at_slices] = refs.view(np.uint8)
    host[at_slices:at_bits] = slice_first.view(np.uint8)
    host[at_bits:] = bits[:need]
    return StagedFrames(stage.to(torch.device(device), non_blocking=True), at_slices, at_bits, int(n_frames), int(refs.size), tuple(shape), affine,
                        int(one), bool(on_scan), path)


def unpack_frames(frames, scan, device=None, roi=None, out: Optional[torch.Tensor] = None) -> DeviceVolume:
    """The frames of one SEG segment -> a uint8 mask (`mmnn_unpack_frames`): 0 / 1 on the grid of `scan` (anything with `.shape` and
    `.affine`) when they lie on it, else 0 / 255 on the segmentation's own stack, marked `from_dicom` so that it is resampled and
    binarised like a DICOM mask series.  `frames`: what `stage_frames` takes, or its result.  One pinned staging buffer, one
    non-blocking copy and one launch on the current stream.  `device`: None is `out`'s, else the current one.  `out`: a contiguous
    uint8 CUDA tensor of the grid's x*y*z elements to write, allocated when None."""
    if not isinstance(frames, StagedFrames):
        frames = stage_frames(frames, scan, _default_device(out) if device is None else device, roi)
    return frames.to_volume(scan, out)


def stage_mask(scan, mask, device):
    """A mask of any source beside `scan` on the device: contours and frames staged (`to_volume` runs their kernel), a volume uploaded."""
    if isinstance(mask, ContourSet):
        return stage_contours(mask, scan, device)
    if isinstance(mask, FrameSet):
        return stage_frames(mask, scan, device)
    return mask if isinstance(mask, (StagedContours, StagedFrames)) else upload(mask, device)


def workspace_bytes(x: int, y: int, z: int) -> int:
    return _lib.count("mmnn_ingest_workspace_bytes", int(x), int(y), int(z))


def resample_mask(mask, scan_shape, index_map, threshold: float = 0.5, out: Optional[torch.Tensor] = None) -> DeviceVolume:
    """Enqueue `mmnn_resample_mask` on the current stream: the mask, drawn on a grid of its own, as uint8 0 / 1 on the scan's grid
    (trilinear blend of the scaled mask voxels in fp64, 1 where it exceeds `threshold`, 0 outside the mask's grid).  `index_map`:
    (3, 4), scan voxel index -> continuous mask index (`nifti.index_map`).  `mask`: DeviceVolume, or a host volume (uploaded to
    `out`'s device, else the current one); `out`: a contiguous uint8 CUDA tensor of x*y*z elements to write, allocated when None."""
    x, y, z = (int(v) for v in scan_shape)
    t = np.ascontiguousarray(np.asarray(index_map, dtype=np.float64))
    if t.shape != (3, 4):
        raise ValueError(f"resample_mask: index_map must be (3, 4), got {t.shape}")
    if not isinstance(mask, DeviceVolume):
        mask = upload(mask, _default_device(out))
    dev = mask.data.device
    if min(x, y, z) >= 1:
        out = _lib.device_buffer(out, x * y * z, torch.uint8, dev, "resample_mask")
    mx, my, mz = mask.shape
    desc = _lib.ResampleMaskDesc(x, y, z, mx, my, mz, mask.datatype, mask.slope, mask.inter, (ctypes.c_double * 12)(*t.reshape(-1)), float(threshold))
    _lib.enqueue("mmnn_resample_mask", ctypes.byref(desc), mask.data.data_ptr(), out.data_ptr() if out is not None else None, device=dev)
    return DeviceVolume(out.view(-1), (x, y, z), TYPE_CODES[np.dtype("uint8")], 1.0, 0.0)


def moved(scan_shape, index_map, tolerance: float = GEOMETRY_TOLERANCE) -> bool:
    """Whether a corner of the scan grid maps more than `tolerance` voxels away from itself under `index_map` (equal extents that do
    not sit on the same grid in space)."""
    t = np.asarray(index_map, dtype=np.float64)
    for corner in np.ndindex(2, 2, 2):
        p = np.array([c * (n - 1) for c, n in zip(corner, scan_shape)], dtype=np.float64)
        if np.linalg.norm(t[:, :3] @ p + t[:, 3] - p) > tolerance:
            return True
    return False


def mask_index_map(scan, mask, mode: str = "auto"):
    """The index map to resample `mask` by under `Data: mask_resample` = `mode`, or None for the voxelwise path.  `scan`, `mask`:
    anything with `.shape` and `.affine`.  Raises ConfigurationError where `mode` or the missing geometry forbids a needed resample."""
    if mode not in MASK_RESAMPLE_MODES:
        raise ConfigurationError(f"mask_resample {mode!r} is none of {MASK_RESAMPLE_MODES}")
    if _placed(scan, mask):
        if isinstance(mask, FrameSet):       # still on the host: placed here as `stage_frames` will place it
            mask = seg.to_scan(mask, scan.shape, scan.affine)
        if getattr(mask, "on_scan", True):   # rasterised or unpacked onto the scan's own grid (a ContourSet always is): nothing to resample
            return None
        if mode == "never":
            raise ConfigurationError(f"scan extent {tuple(scan.shape)} ({getattr(scan, 'path', '') or 'scan'}), SEG extent {tuple(mask.shape)} "
                                     f"({mask.path or 'mask'}): the segmentation is on a grid of its own and mask_resample is 'never'")
        return nifti.index_map(scan, mask)
    same = tuple(scan.shape) == tuple(mask.shape)
    if is_dicom(scan) or is_dicom(mask):
        return _dicom_index_map(scan, mask, mode, same)
    if same:
        if mode != "geometry" or scan.affine is None or mask.affine is None:
            return None
        t = nifti.index_map(scan, mask)
        return t if moved(scan.shape, t) else None
    if mode == "never":
        raise ConfigurationError(f"scan extent {tuple(scan.shape)} differs from the mask's {tuple(mask.shape)} and mask_resample is 'never'")
    return nifti.index_map(scan, mask)


def _placed(scan, mask, named=False) -> bool:
    """Whether `mask` is contours or frames, placed against its scan's geometry, rather than a volume with a grid of its own.  Beside
    a scan that is no DICOM series they are refused here (`named`: with their file)."""
    rs, sg = "an RTSTRUCT mask", "a DICOM SEG mask"
    what = {ContourSet: rs, StagedContours: rs, FrameSet: sg, StagedFrames: sg, seg.Placement: sg}.get(type(mask))
    if what and not is_dicom(scan):
        raise ConfigurationError(f"{what}{f' ({mask.path})' if named else ''} beside a NIfTI scan is outside the path: both come from one format")
    return what is not None


def is_dicom(volume) -> bool:
    return isinstance(volume, DicomSeries) or bool(getattr(volume, "from_dicom", False))


def default_threshold(scan) -> float:
    """The `mask_threshold` a pair is binarised at when none is configured: 128 behind a DICOM scan (upstream's `mask > 128`), else 0.5."""
    return DICOM_MASK_THRESHOLD if is_dicom(scan) else NIFTI_MASK_THRESHOLD


def _dicom_index_map(scan, mask, mode, same):
    """A DICOM pair is always resampled: by the two geometries, by the identity when they are one grid bit for bit, or -- a series
    without geometry (a single slice without position) -- by the identity when the extents agree."""
    if not (is_dicom(scan) and is_dicom(mask)):
        raise ConfigurationError("a NIfTI mask beside a DICOM scan (or the reverse) is outside the path: both come from one format")
    what = f"scan extent {tuple(scan.shape)} ({getattr(scan, 'path', '') or 'scan'}), mask extent {tuple(mask.shape)} ({getattr(mask, 'path', '') or 'mask'})"
    if not same and mode == "never":
        raise ConfigurationError(what + ": they differ and mask_resample is 'never'")
    if scan.affine is None or mask.affine is None:
        if not same:
            raise ConfigurationError(what + ": they differ and a series has no geometry to resample by")
        return IDENTITY_MAP
    if same and np.array_equal(np.asarray(scan.affine), np.asarray(mask.affine)):
        return IDENTITY_MAP
    return nifti.index_map(scan, mask)


def prepare_pair(scan, mask, dev, index_map=None, threshold: Optional[float] = None, what: str = "ingest"):
    """The front that every consumer of a (scan, mask) pair shares (`ingest_volume`, `radiomics.extract`): upload what is still on the
    host, rasterise an RTSTRUCT mask, unpack a SEG mask, resample a mask drawn on another grid (binarised at `threshold`; None: 0.5, or
    128 behind a DICOM scan).  Returns (scan, mask), two DeviceVolumes on one grid.  The rules are `ingest_volume`'s."""
    scan = upload(scan, dev)
    drawn = _placed(scan, mask)
    mask = stage_mask(scan, mask, dev)
    if drawn:
        drawn = mask.on_scan                 # on the scan's grid: the voxelwise path; on its own: a DICOM mask volume like a series'
        if drawn and index_map is not None:
            raise ValueError(f"{what}: {mask.no_index_map}")
        mask = mask.to_volume(scan)
    if threshold is None:
        threshold = default_threshold(scan)
    if index_map is None and not drawn and (is_dicom(scan) or is_dicom(mask)):
        index_map = mask_index_map(scan, mask)
    if index_map is None and scan.shape != mask.shape:
        if scan.affine is None or mask.affine is None:
            raise ValueError(f"{what}: scan extent {scan.shape} differs from the mask's {mask.shape}")
        index_map = nifti.index_map(scan, mask)
    if index_map is not None:
        mask = resample_mask(mask, scan.shape, index_map, threshold)
    return scan, mask


MARGIN_MODES = {"dilate": _lib.MARGIN_DILATE, "shell": _lib.MARGIN_SHELL}


def margin_radius(radius_mm, key: str = "mask_margin_mm"):
    """`radius_mm` as a margin in mm: None stays None (the step is off), otherwise a positive finite number, else ConfigurationError."""
    if radius_mm is None:
        return None
    try:
        r = float("nan") if isinstance(radius_mm, bool) else float(radius_mm)
    except (TypeError, ValueError):
        r = float("nan")
    if not (r > 0.0 and r < float("inf")):
        raise ConfigurationError(f"{key} must be a positive finite number of mm, got {radius_mm!r}")
    return r


def margin_reach(spacing, radius_mm) -> Tuple[int, int, int]:
    """`mmnn_mask_margin_reach`: per axis the largest index distance k with (k s_a)^2 <= radius^2, on the host (no GPU).  ValueError for a
    spacing or radius that is not finite and > 0 and for a reach above the library's cap (`_lib.MARGIN_MAX_REACH`)."""
    s = (ctypes.c_double * 3)(*(float(v) for v in spacing))
    reach = (ctypes.c_int32 * 3)()
    _lib.call("mmnn_mask_margin_reach", s, float(radius_mm), reach)
    return tuple(int(v) for v in reach)


def mask_margin_workspace_bytes(x: int, y: int, z: int) -> int:
    return _lib.count("mmnn_mask_margin_workspace_bytes", int(x), int(y), int(z))


def mask_margin(mask: DeviceVolume, spacing, radius_mm, mode: str = "dilate", out: Optional[torch.Tensor] = None,
                dist2: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> DeviceVolume:
    """Enqueue `mmnn_mask_margin` on the current stream of the mask's device: the mask widened by `radius_mm` under the voxel `spacing`
    (x, y, z in mm; `radiomics.spacing_of(scan.affine)`, the column norms of the affine's linear part, (1, 1, 1) without an affine).
    `mode` 'dilate': 1 where the exact Euclidean distance to the nearest set voxel is <= radius_mm (the mask plus its rim); 'shell': 1
    where it is > 0 and <= radius_mm (the rim alone).  A voxel is set when its scaled value is not 0, as the ingest reads a mask.
    The distance treats the index axes as orthogonal, which those of a sheared affine are not; shear is not detected.
    `mask`: a DeviceVolume on the scan's grid (what `prepare_pair` returns).  `out`: a contiguous uint8 tensor of x*y*z elements on its
    device to write, which must not be the mask's own; `dist2`: None, or x*y*z contiguous float64 that receive the squared distance in
    mm^2 where it is <= radius^2 and +inf elsewhere; `workspace`: at least `mask_margin_workspace_bytes` of uint8.  `out` and
    `workspace` are allocated when None.  The result has type 2, slope 1, inter 0 and the mask's affine (on this path the scan's).
    A radius smaller than every spacing reaches no neighbour -- the dilation would be the mask and the shell empty -- and is refused."""
    if mode not in MARGIN_MODES:
        raise ValueError(f"mask_margin: mode {mode!r} is none of {tuple(MARGIN_MODES)}")
    if not isinstance(mask, DeviceVolume):
        raise ValueError("mask_margin: the mask must be a DeviceVolume on the scan's grid (see prepare_pair)")
    spacing = tuple(float(v) for v in spacing)
    if len(spacing) != 3:
        raise ValueError(f"mask_margin: spacing must be three numbers (x, y, z in mm), got {spacing!r}")
    reach = margin_reach(spacing, radius_mm)
    if reach == (0, 0, 0):
        raise ValueError(f"mask_margin: a radius of {float(radius_mm)} mm is smaller than every voxel spacing ({spacing[0]}, {spacing[1]}, "
                         f"{spacing[2]} mm): it reaches no neighbouring voxel, so the dilation is the mask itself and the shell is empty")
    dev = mask.data.device
    x, y, z = (int(v) for v in mask.shape)
    n = x * y * z
    if min(x, y, z) >= 1:
        out = _lib.device_buffer(out, n, torch.uint8, dev, "mask_margin")
        if dist2 is not None:
            dist2 = _lib.device_buffer(dist2, n, torch.float64, dev, "mask_margin (dist2)")
        workspace = _lib.workspace(workspace, mask_margin_workspace_bytes(x, y, z), dev, "mask_margin")
    desc = _lib.MaskMarginDesc(x, y, z, mask.datatype, float(mask.slope), float(mask.inter), (ctypes.c_double * 3)(*spacing), float(radius_mm),
                               MARGIN_MODES[mode])
    _lib.enqueue("mmnn_mask_margin", ctypes.byref(desc), mask.data.data_ptr(), None if out is None else out.data_ptr(),
                 None if dist2 is None else dist2.data_ptr(), None if workspace is None else workspace.data_ptr(), device=dev)
    return DeviceVolume(out.view(-1), (x, y, z), TYPE_CODES[np.dtype("uint8")], 1.0, 0.0, mask.affine)


def widen_mask(scan: DeviceVolume, mask: DeviceVolume, radius_mm, mode: str = "dilate") -> DeviceVolume:
    """`mask_margin` of a prepared pair's mask under the spacing of the scan's affine; the result carries the scan's affine."""
    from .. import radiomics
    out = mask_margin(mask, radiomics.spacing_of(scan.affine), radius_mm, mode)
    out.affine = scan.affine
    return out


def check_size(size, who: str = "ingest") -> int:
    """`size` as an output extent per axis: an integer in 1..MAX_SIZE, else ValueError."""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= int(size) <= MAX_SIZE:
        raise ValueError(f"{who}: the output extent per axis must be an integer in 1..{MAX_SIZE}, got {size!r}")
    return int(size)


def ingest_volume(scan, mask, out_plane: torch.Tensor, extents: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                  index_map=None, threshold: Optional[float] = None, mask_margin_mm: Optional[float] = None) -> torch.Tensor:
    """Enqueue the ingest of one volume on the current stream: `out_plane` (a contiguous (S,S,S) fp32 CUDA view with S in 1..128, e.g. batch[n, c]) receives
    the masked, compacted scan, area-resized to S^3; returns `extents` (3 x int32 on the device: kept slices along x, y, z), readable after
    the next synchronisation.  `scan` / `mask`: DeviceVolume, NiftiImage or ndarray (host volumes are uploaded first).  When the
    extents differ, or an `index_map` is given, the mask is first resampled into the scan's grid (`resample_mask`, binarised at
    `threshold`); without `index_map` the map comes from the two volumes' affines, and differing extents without them are refused.
    Equal extents without `index_map` are the voxelwise path -- except for a DICOM pair, which is always resampled.  `threshold`
    None: 0.5, or 128 behind a DICOM scan.  A `mask` that is a ContourSet (or `stage_contours`' result) beside a DICOM scan is
    rasterised onto the scan's grid first (`rasterize_contours`) and takes the voxelwise path: no resample, no threshold.  A `mask`
    that is a FrameSet (or `stage_frames`' result) beside a DICOM scan is unpacked first (`unpack_frames`): onto the scan's grid, and
    then voxelwise like a contour mask, or onto a grid of its own, and then resampled and binarised like a DICOM mask series.
    `mask_margin_mm` (None: nothing is launched or allocated for it): behind all of that the mask is replaced by its dilation by that many
    mm (`mask_margin`, under the spacing of the scan's affine) and the ingest runs unchanged on it: the plane is scan x (1 inside tumour +
    margin, 0 outside) and the slices the rim touches are kept.  The dilated mask is 0 / 1, so a mask whose set voxels hold another value
    (255) no longer scales the plane by it."""
    shape = tuple(out_plane.shape)
    if not (out_plane.is_cuda and out_plane.dtype == torch.float32 and out_plane.is_contiguous() and len(shape) == 3
            and shape == shape[:1] * 3 and 1 <= shape[0] <= MAX_SIZE):
        raise ValueError(f"ingest: out_plane must be a contiguous ({SIZE},{SIZE},{SIZE}) fp32 CUDA tensor, or (S,S,S) with another S in 1..{MAX_SIZE}, "
                         f"got {shape} {out_plane.dtype} on {out_plane.device}")
    size = shape[0]
    dev = out_plane.device
    scan, mask = prepare_pair(scan, mask, dev, index_map, threshold)
    if mask_margin_mm is not None:
        mask = widen_mask(scan, mask, mask_margin_mm)
    extents = _lib.device_buffer(extents, 3, torch.int32, dev, "ingest (extents)")
    x, y, z = scan.shape
    workspace = _lib.workspace(workspace, workspace_bytes(x, y, z), dev, "ingest")
    desc = _lib.IngestDesc(x, y, z, scan.datatype, mask.datatype, scan.slope, scan.inter, mask.slope, mask.inter)
    _lib.enqueue("mmnn_ingest_volume_sized", ctypes.byref(desc), size, scan.data.data_ptr(), mask.data.data_ptr(), out_plane.data_ptr(),
                 extents.data_ptr(), workspace.data_ptr(), device=dev)
    return extents


def maps_to_scan_workspace_bytes(x: int, y: int, z: int) -> int:
    return _lib.count("mmnn_maps_to_scan_workspace_bytes", int(x), int(y), int(z))


def maps_to_scan(maps: torch.Tensor, scan_shape, ingest_workspace: torch.Tensor, out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Enqueue `mmnn_maps_to_scan_sized` on the current stream: `maps` ((n_maps, S, S, S) fp32 in model space with S in 1..128, axes
    x, y, z as the ingest writes its plane) -> (n_maps, z, y, x) fp32 on the scan's voxel grid (x fastest, NIfTI order; `.permute(0, 3, 2, 1)` is the (x, y, z)
    array of a volume).  Kept voxels hold the trilinear up-sampling of the map to the kept extents, every voxel of a slice the ingest
    dropped is exactly 0.  `ingest_workspace`: the `workspace` tensor a completed `ingest_volume` of this scan used, not reused since;
    it holds the scan's kept slices and nothing of the extent they were resized to, so S is the maps' own and need not equal that ingest's.
    `out`: a contiguous (n_maps, z, y, x) fp32 tensor on the maps' device to write, allocated when None; `workspace`: scratch of
    `maps_to_scan_workspace_bytes` bytes, allocated when None."""
    shape = tuple(scan_shape)
    if len(shape) != 3 or any(int(v) != v or int(v) < 1 for v in shape):
        raise ValueError(f"maps_to_scan: scan_shape must be three positive extents (x, y, z), got {scan_shape!r}")
    x, y, z = (int(v) for v in shape)
    if (not isinstance(maps, torch.Tensor) or maps.ndim != 4 or tuple(maps.shape[1:]) != tuple(maps.shape[1:2]) * 3
            or not 1 <= maps.shape[1] <= MAX_SIZE or not 1 <= maps.shape[0] <= _lib.MAPS_TO_SCAN_MAX_MAPS):
        raise ValueError(f"maps_to_scan: maps must be (n, {SIZE}, {SIZE}, {SIZE}), or (n, S, S, S) with another S in 1..{MAX_SIZE}, with n in "
                         f"1..{_lib.MAPS_TO_SCAN_MAX_MAPS}, got {tuple(getattr(maps, 'shape', ()))}")
    if maps.dtype != torch.float32 or not maps.is_contiguous():
        raise ValueError(f"maps_to_scan: maps must be contiguous fp32, got {maps.dtype}{'' if maps.is_contiguous() else ' (not contiguous)'}")
    if not isinstance(ingest_workspace, torch.Tensor) or ingest_workspace.dtype != torch.uint8 or not ingest_workspace.is_contiguous():
        raise ValueError("maps_to_scan: ingest_workspace must be the contiguous uint8 workspace tensor of the scan's ingest")
    if not maps.is_cuda:
        raise ValueError(f"maps_to_scan: maps must be on the GPU, got {maps.device}")
    dev = maps.device
    if ingest_workspace.device != dev:
        raise ValueError(f"maps_to_scan: ingest_workspace is on {ingest_workspace.device}, the maps on {dev}")
    n = int(maps.shape[0])
    out = _lib.device_buffer(out, (n, z, y, x), torch.float32, dev, "maps_to_scan")
    if ingest_workspace.numel() < workspace_bytes(x, y, z):
        raise ValueError(f"maps_to_scan: ingest_workspace of {ingest_workspace.numel()} bytes, an ingest of {x} x {y} x {z} leaves {workspace_bytes(x, y, z)}")
    workspace = _lib.workspace(workspace, maps_to_scan_workspace_bytes(x, y, z), dev, "maps_to_scan")
    desc = _lib.MapsToScanDesc(x, y, z, n)
    _lib.enqueue("mmnn_maps_to_scan_sized", ctypes.byref(desc), int(maps.shape[1]), ingest_workspace.data_ptr(), maps.data_ptr(), out.data_ptr(),
                 workspace.data_ptr(), device=dev)
    return out


def collate_volumes(patients: Sequence[Sequence[Tuple[object, object]]], device, mask_resample: str = "auto",
                    mask_threshold: Optional[float] = None, keep_workspaces: bool = False, size: int = SIZE,
                    mask_margin_mm: Optional[float] = None):
    """patients[n][c] = (scan, mask) -> the device batch (N, C, S, S, S) fp32, S = `size` in 1..128, and the kept extents (N, C, 3) int32.  Every upload is
    issued before the first kernel, so the copies of one volume run beside the passes of the one before it.  A mask on another grid
    than its scan's is resampled first, as `mask_resample` ('auto', 'geometry', 'never') says, and binarised at `mask_threshold`
    (None: 0.5; 128 for a DICOM pair, which is always resampled).  A ContourSet as the mask of a DICOM scan (an RTSTRUCT file) is
    placed on that scan's grid by the host, uploaded with the others and rasterised there; it takes neither resample nor threshold.
    A FrameSet (a DICOM SEG file) is placed by the host, uploaded with the others and unpacked on the device (see `unpack_frames`).
    With `keep_workspaces` every volume is ingested with a workspace of its own and a third value is returned: volumes[n][c], the
    `KeptVolume` (workspace, scan extents, scan affine) that `maps_to_scan` needs to lay a map of the model over that scan.
    `mask_margin_mm` (`Data: mask_margin_mm`; None: off): every mask is replaced by its dilation by that many mm ahead of the ingest (see
    `ingest_volume`); the kept lists, and with them the maps `maps_to_scan` lays back, are those of the widened box."""
    size = check_size(size)
    n, c = len(patients), len(patients[0])
    if any(len(p) != c for p in patients):
        raise ValueError("ingest: patients of one batch differ in their number of modalities")
    device = torch.device(device)
    batch = torch.empty((n, c, size, size, size), dtype=torch.float32, device=device)
    extents = torch.empty((n, c, 3), dtype=torch.int32, device=device)
    margin = {} if mask_margin_mm is None else {"mask_margin_mm": mask_margin_mm}      # (without one the call is the one it always was)
    kept = ingest_patients(patients, device, [(batch[i], extents[i]) for i in range(n)], mask_resample, mask_threshold, keep_workspaces, **margin)
    return (batch, extents, kept) if keep_workspaces else (batch, extents)


def ingest_patients(patients, device, into, mask_resample: str = "auto", mask_threshold: Optional[float] = None, keep_workspaces: bool = False,
                    mask_margin_mm: Optional[float] = None):
    """The uploads and launches of `collate_volumes` with the destinations named by the caller: into[n] = (planes (C, S, S, S) fp32,
    extents (C, 3) int32), two contiguous device views that patient n is ingested into -- a row of a batch, or a row of the volume
    cache (`mmnn_sts_amd.data.cache`).  Returns the `KeptVolume`s, volumes[n][c] (empty lists without `keep_workspaces`).
    `mask_margin_mm`: as in `collate_volumes`."""
    mask_margin_mm = margin_radius(mask_margin_mm)
    margin = {} if mask_margin_mm is None else {"mask_margin_mm": mask_margin_mm}
    up = [[(upload(s, device), stage_mask(s, m, device)) for s, m in p] for p in patients]
    maps = [[mask_index_map(s, m, mask_resample) for s, m in p] for p in up]
    kept = []
    for i, (planes, extents) in enumerate(into):
        kept.append([])
        for j in range(len(up[i])):
            ws = torch.empty(workspace_bytes(*up[i][j][0].shape), dtype=torch.uint8, device=device) if keep_workspaces else None
            ingest_volume(up[i][j][0], up[i][j][1], planes[j], extents[j], ws, index_map=maps[i][j], threshold=mask_threshold, **margin)
            if keep_workspaces:
                kept[i].append(KeptVolume(ws, up[i][j][0].shape, up[i][j][0].affine))
    return kept


class IngestCollate:
    """collate_fn of the NIfTI and DICOM datasets: items are (x, events, durations) or (x, labels) with x a RawPatient or
    {'image': RawPatient, 'clinical': tensor}; returns (x, events, durations) (durations None for classification items) with the image
    batch on `device`.  The extents of every batch are kept in `pending` until `take_empty()` reads them: call it where the epoch
    synchronises anyway, never per batch.  `mask_resample` / `mask_threshold`: the `Data:` keys of the same names (see `collate_volumes`).
    `keep_workspaces` (off: nothing is retained, as training wants it): `last_volumes[n][c]` holds the `KeptVolume` of every (patient,
    modality) of the LAST batch, for `maps_to_scan`.  `size`: the extent S per axis of the planes, 1..128 (64).
    `cache` (None: every patient is ingested into every batch it is in): a `VolumeCache` (`mmnn_sts_amd.data.cache`) of this device,
    size and channel count.  A patient seen for the first time is then ingested straight into its row of the cache -- the same calls
    with another destination -- and every batch is assembled from the cache's rows by `mmnn_gather_rows` on the same stream, so batch
    and extents hold the bits they hold without a cache; an item whose image is a `CachedPatient` brings no voxels at all.  A patient
    that found the cache full is ingested into its row of the batch, as without one.
    `mask_margin_mm` (`Data: mask_margin_mm`, `--mask_margin_mm`; None: off, and every batch is bit for bit what it is without the
    key): every mask is dilated by that many mm on the device ahead of its ingest; a cache then stores what that ingest made."""

    def __init__(self, device, mask_resample: str = "auto", mask_threshold: Optional[float] = 0.5, keep_workspaces: bool = False,
                 size: int = SIZE, cache=None, mask_margin_mm: Optional[float] = None):
        if mask_resample not in MASK_RESAMPLE_MODES:
            raise ConfigurationError(f"mask_resample {mask_resample!r} is none of {MASK_RESAMPLE_MODES}")
        self.device = torch.device(device)
        self.mask_resample, self.mask_threshold = mask_resample, (None if mask_threshold is None else float(mask_threshold))
        self.pending: List[Tuple[List[int], torch.Tensor]] = []
        self.keep_workspaces = bool(keep_workspaces)
        self.size = check_size(size)
        self.mask_margin_mm = margin_radius(mask_margin_mm)
        self.last_volumes: List[List[KeptVolume]] = []
        if cache is not None and self.keep_workspaces:
            raise ConfigurationError("a volume cache keeps no ingest workspaces: keep_workspaces (inference, which reads each patient once) excludes it")
        held = None if cache is None else cache.planes.device
        if cache is not None and (cache.size != self.size or held.type != self.device.type or self.device.index not in (None, held.index)):
            raise ConfigurationError(f"the volume cache holds {cache.size}^3 planes on {cache.planes.device}, the collate makes {self.size}^3 ones on {self.device}")
        self.cache = cache

    def __call__(self, items):
        xs = [it[0] for it in items]
        targets = [torch.stack([torch.as_tensor(it[k]) for it in items]) for k in range(1, len(items[0]))]
        multimodal = isinstance(xs[0], dict)
        raws = [x["image"] for x in xs] if multimodal else xs
        if self.cache is not None:
            batch, extents = self._through_cache(raws)
        else:
            sized = {"size": self.size} if self.size != SIZE else {}      # (the default's call is the one it always was)
            if self.mask_margin_mm is not None:
                sized["mask_margin_mm"] = self.mask_margin_mm
            batch, extents, *kept = collate_volumes([r.volumes for r in raws], self.device, self.mask_resample, self.mask_threshold,
                                                    keep_workspaces=self.keep_workspaces, **sized)
            if kept:
                self.last_volumes = kept[0]
        self.pending.append(([r.uid for r in raws], extents))
        x = {"image": batch, "clinical": torch.stack([x["clinical"] for x in xs]).float()} if multimodal else batch
        return (x, targets[0], targets[1] if len(targets) > 1 else None)

    def _through_cache(self, raws):
        """The batch of `raws` (RawPatient or CachedPatient each) with the cache between the ingest and the batch.  One gather per run of
        adjacent cached rows: one for a batch without an overflow patient."""
        cache, n = self.cache, len(raws)
        batch = torch.empty((n, cache.channels, self.size, self.size, self.size), dtype=torch.float32, device=self.device)
        extents = torch.empty((n, cache.channels, 3), dtype=torch.int32, device=self.device)
        slots, cold, into = [None] * n, [], []
        for i, r in enumerate(raws):
            if cache.filled(r.uid):
                slots[i] = cache.table.hit(r.uid)
                continue
            volumes = getattr(r, "volumes", None)
            if volumes is None:
                raise ValueError(f"ingest: patient uid {r.uid} arrived without voxels and is not in the volume cache")
            if len(volumes) != cache.channels:
                raise ValueError(f"ingest: patient uid {r.uid} has {len(volumes)} modalities, the volume cache holds {cache.channels} channels")
            slots[i] = cache.table.assign(r.uid)
            cold.append((r.uid, volumes, slots[i]))
            into.append((batch[i], extents[i]) if slots[i] is None else (cache.planes[slots[i]], cache.extents[slots[i]]))
        if cold:
            margin = {} if self.mask_margin_mm is None else {"mask_margin_mm": self.mask_margin_mm}
            ingest_patients([v for _, v, _ in cold], self.device, into, self.mask_resample, self.mask_threshold, **margin)
            for uid, _, slot in cold:
                if slot is not None:
                    cache.table.mark_filled(uid)
        i = 0
        while i < n:
            j = i
            while j < n and slots[j] is not None:
                j += 1
            if j > i:
                cache.gather(slots[i:j], batch[i:j], extents[i:j])
            i = max(j, i + 1)
        return batch, extents

    def take_empty(self) -> List[int]:
        """uids (sorted, each once) of the patients seen since the last call whose mask left nothing of a scan (an extent of 0)."""
        bad = set()
        for uids, ext in self.pending:
            hit = (ext.cpu() == 0).any(dim=2).any(dim=1).tolist()
            bad.update(u for u, h in zip(uids, hit) if h)
        self.pending = []
        return sorted(bad)
