"""A minimal DICOM Segmentation (SEG) reader (numpy and struct only, on `dicom.py`'s file opener, nested data-set walk and value
helpers, as `rtstruct.py` is): the bit-packed frames of a BINARY segmentation, which segment and which plane each of them belongs to,
and their placement against a scan's voxel grid for the device unpacker (`mmnn_sts_amd.data.ingest.unpack_frames`, `mmnn_unpack_frames`).  The
host parses the file and places planes; it never looks at a bit of PixelData.

A SEG file is a part-10 file of SOP class 1.2.840.10008.5.1.4.1.1.66.4 (PS3.3 A.51, C.8.20), an enhanced multi-frame object:

    Rows (0028,0010), Columns (0028,0011), NumberOfFrames (0028,0008), BitsAllocated (0028,0100), SegmentationType (0062,0001)
    SegmentSequence (0062,0002)                       per segment: SegmentNumber (0062,0004), SegmentLabel (0062,0005)
    SharedFunctionalGroupsSequence (5200,9229)        one item; PerFrameFunctionalGroupsSequence (5200,9230): one item per frame, with
        PlaneOrientationSequence (0020,9116)          -> ImageOrientationPatient (0020,0037)        shared, or in every per-frame item
        PixelMeasuresSequence (0028,9110)             -> PixelSpacing, SliceThickness, SpacingBetweenSlices      (the same)
        PlanePositionSequence (0020,9113)             -> ImagePositionPatient (0020,0032)           per frame
        SegmentIdentificationSequence (0062,000A)     -> ReferencedSegmentNumber (0062,000B)        per frame
    PixelData (7FE0,0010)                             one bit per pixel, least significant bit first (PS3.5 8.2, Annex D), the frames
                                                      back to back WITHOUT byte alignment: ceil(frames * rows * columns / 8) bytes

in explicit or implicit VR little endian, with sequences and items of defined or undefined length.  Only the planes a segment touches
are stored; they come in any order and several segments share one file.  Refused, with the file named: another SOP class,
SegmentationType FRACTIONAL or LABELMAP and BitsAllocated other than 1, every transfer syntax `dicom.py` refuses (RLE-compressed SEG is
common: decompress the file first), a truncated PixelData, a frame count that disagrees with the per-frame items, a frame without
position or segment number, a file without orientation.

    read(path, header_only=False)                 -> FrameSet: segment labels in file order and, per frame, its segment and plane
    select(frame_set, roi)                        -> the FrameSet of one segment (label match exact, case-insensitive; None: the only one)
    to_scan(frames, scan_shape, scan_affine)      -> Placement: refs / slice_first for `mmnn_unpack_frames`, on the scan's grid when the
                                                     frames lie on its slice planes, else on a stack of the segmentation's own

Parity with GDCM / SimpleITK / highdicom is unpinned: none is installed where this was written.  The path is pinned to PS3.3 C.8.20,
to the PS3.5 bit order stated above `mmnn_unpack_frames` in the header, and to the NIfTI twin
(`synth_dicom.from_nifti_tree(..., mask_format="seg")` must give the same device batch as the NIfTI tree, bit for bit).  Enhanced
multi-frame *scans*, FRACTIONAL and LABELMAP SEG and compressed syntaxes stay outside the path.
"""
import dataclasses
import logging
import struct
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from ..exceptions.exceptions import ConfigurationError
from .dicom import (PIXEL_DATA, UNDEFINED, _check_syntax, _element, _floats, _integer, _refuse, _skip_sequence, _text, lps_to_ras, match_name,
                    part10, walk)

logger = logging.getLogger(__name__)

SEGMENTATION_STORAGE = "1.2.840.10008.5.1.4.1.1.66.4"
SOP_CLASS_UID = (0x0008, 0x0016)
NUMBER_OF_FRAMES, ROWS, COLUMNS, BITS_ALLOCATED = (0x0028, 0x0008), (0x0028, 0x0010), (0x0028, 0x0011), (0x0028, 0x0100)
SEGMENTATION_TYPE, SEGMENT_SEQUENCE, SEGMENT_NUMBER, SEGMENT_LABEL = (0x0062, 0x0001), (0x0062, 0x0002), (0x0062, 0x0004), (0x0062, 0x0005)
SHARED_GROUPS, PER_FRAME_GROUPS = (0x5200, 0x9229), (0x5200, 0x9230)
PLANE_ORIENTATION, PIXEL_MEASURES, PLANE_POSITION, SEGMENT_IDENTIFICATION = (0x0020, 0x9116), (0x0028, 0x9110), (0x0020, 0x9113), (0x0062, 0x000A)
ORIENTATION, POSITION, PIXEL_SPACING, SLICE_THICKNESS, SPACING_BETWEEN = (0x0020, 0x0037), (0x0020, 0x0032), (0x0028, 0x0030), (0x0018, 0x0050), (0x0018, 0x0088)
REFERENCED_SEGMENT_NUMBER = (0x0062, 0x000B)
ENTERED = frozenset((SEGMENT_SEQUENCE, SHARED_GROUPS, PER_FRAME_GROUPS, PLANE_ORIENTATION, PIXEL_MEASURES, PLANE_POSITION, SEGMENT_IDENTIFICATION))
KEPT = frozenset((SOP_CLASS_UID, NUMBER_OF_FRAMES, ROWS, COLUMNS, BITS_ALLOCATED, SEGMENTATION_TYPE, SEGMENT_NUMBER, SEGMENT_LABEL, ORIENTATION,
                  POSITION, PIXEL_SPACING, SLICE_THICKNESS, SPACING_BETWEEN, REFERENCED_SEGMENT_NUMBER))
ON_GRID_TOLERANCE = 1e-3                     # voxels (= ingest.GEOMETRY_TOLERANCE): how far a frame's corners may lie from the scan's lattice
ORIENTATION_TOLERANCE = 1e-4                 # as dicom._geometry compares ImageOrientationPatient
IN_PLANE_TOLERANCE = 1e-3                    # voxels: in-plane offset between the frames of a stack
STEP_TOLERANCE = 0.01                        # steps: distance of a frame from a whole multiple of the slice step
_warned = set()                              # files whose dropped frames have been reported


@dataclass
class FrameSet:
    """The frames of one file.  `names`: SegmentLabel in file order; `segment_of[f]`: the index into `names` of frame f's segment (-1:
    a segment that `select` left out); `positions` (F, 3), `orientations` (F, 6): ImagePositionPatient / ImageOrientationPatient per
    frame, LPS; `spacings` (F, 2): PixelSpacing per frame (row spacing, column spacing; NaN where the file has none); `steps` (F,):
    SpacingBetweenSlices, else SliceThickness, per frame (NaN: neither); `frame`: a zero-copy uint8 view of the
    ceil(F * rows * columns / 8) PixelData bytes (None with header_only)."""
    path: str
    names: List[str]
    rows: int
    columns: int
    segment_of: np.ndarray
    positions: np.ndarray
    orientations: np.ndarray
    spacings: np.ndarray
    steps: np.ndarray
    frame: Optional[np.ndarray] = None
    header_only: bool = False

    @property
    def n_frames(self):
        return int(len(self.segment_of))


@dataclass
class Placement:
    """Where the frames of one segment go (`to_scan`).  `shape`, `affine`: the grid `mmnn_unpack_frames` writes -- the scan's own
    (`on_scan`), or the segmentation's stack with one empty slice on either side and its RAS voxel-index -> mm matrix; `refs`,
    `slice_first`: int32 arrays of the C-ABI; `one`: 1 on the scan's grid (the voxelwise path), 255 on a grid of its own (resampled and
    binarised like a DICOM mask series); `dropped`: frames that lie outside the scan's slices."""
    shape: Tuple[int, int, int]
    affine: np.ndarray
    refs: np.ndarray
    slice_first: np.ndarray
    one: int
    on_scan: bool
    dropped: int = 0
    path: str = ""
    from_dicom: bool = True


def sop_class_of(path) -> Optional[str]:
    """SOPClassUID (0008,0016) of a part-10 file from its first elements alone, or None (NotDicomError without the magic).  What the
    datasets tell a SEG file from an image or an RTSTRUCT file by, before any reader validates it."""
    with part10(path) as f:
        path, buf, size, syntax, off = f.path, f.buf, f.size, f.syntax, f.off
        explicit = syntax != "1.2.840.10008.1.2"      # (every syntax but implicit VR little endian is explicit; only the tag order matters here)
        if syntax == "1.2.840.10008.1.2.2":           # big endian: the data set cannot be walked little endian; the meta group names the class too
            return _media_storage_class(buf, path)
        while off + 8 <= size:
            tag, vr, length, voff = _element(buf, off, explicit, path)
            if tag > SOP_CLASS_UID or tag[0] == 0xFFFE:
                break
            if tag == SOP_CLASS_UID and length != UNDEFINED and voff + length <= size:
                return _text(buf, (voff, length)) or None
            if length == UNDEFINED:
                off = _skip_sequence(buf, voff, explicit and vr != "UN", path)
            else:
                off = voff + length
        return _media_storage_class(buf, path)


def _media_storage_class(buf, path):
    """MediaStorageSOPClassUID (0002,0002) of the file meta group, or None."""
    off = 132
    while off + 8 <= len(buf) and struct.unpack_from("<H", buf, off)[0] == 0x0002:
        tag, _, length, voff = _element(buf, off, True, path)
        if length == UNDEFINED:
            return None
        if tag == (0x0002, 0x0002):
            return _text(buf, (voff, length)) or None
        off = voff + length
    return None


def _group(buf, item, tag, inner, what, count, path):
    """The numbers of element `inner` inside the first item of functional group `tag` of `item`, or None."""
    seq = item.get(tag)
    if not seq or inner not in seq[0]:
        return None
    return _floats(buf, seq[0][inner], what, count, path)


def read(path, header_only=False) -> FrameSet:
    """Parse a SEG file.  With `header_only` the walk stops in front of PixelData: `frame` stays None and its length is not checked."""
    with part10(path) as part:
        path, buf, size, syntax = part.path, part.buf, part.size, part.syntax
        if syntax == "1.2.840.10008.1.2.5":
            _refuse(path, f"transfer syntax {syntax} (RLE lossless, an encapsulated, compressed syntax) is outside the path: only uncompressed "
                          "little endian files are read; decompress the file first")
        explicit, _ = _check_syntax(syntax, path)
        top, _ = walk(buf, part.off, size, explicit, path, KEPT, ENTERED, pixel_data=True)
        sop = _text(buf, top[SOP_CLASS_UID]) if SOP_CLASS_UID in top else None
        if sop != SEGMENTATION_STORAGE:
            _refuse(path, f"SOPClassUID {sop} is not Segmentation Storage ({SEGMENTATION_STORAGE})")
        kind = _text(buf, top[SEGMENTATION_TYPE]).upper() if SEGMENTATION_TYPE in top else ""
        bits = _integer(buf, top[BITS_ALLOCATED], "BitsAllocated", path, "US") if BITS_ALLOCATED in top else None
        if kind in ("FRACTIONAL", "LABELMAP"):
            _refuse(path, f"SegmentationType {kind} is outside the path: only one bit per pixel is unpacked; export as BINARY")
        if kind != "BINARY" or bits != 1:
            _refuse(path, f"SegmentationType {kind or None}, BitsAllocated {bits}: only a BINARY segmentation of one bit per pixel is read; export as BINARY")
        for tag, what in ((ROWS, "Rows"), (COLUMNS, "Columns"), (NUMBER_OF_FRAMES, "NumberOfFrames")):
            if tag not in top:
                _refuse(path, f"no {what} ({tag[0]:04X},{tag[1]:04X})")
        rows, columns = (_integer(buf, top[t], w, path, "US") for t, w in ((ROWS, "Rows"), (COLUMNS, "Columns")))
        n_frames = _integer(buf, top[NUMBER_OF_FRAMES], "NumberOfFrames", path, "IS")
        if rows < 1 or columns < 1 or n_frames < 1:
            _refuse(path, f"Rows {rows}, Columns {columns}, NumberOfFrames {n_frames}")
        segments = top.get(SEGMENT_SEQUENCE, [])
        if not segments:
            _refuse(path, "no SegmentSequence (0062,0002): the segmentation describes no segment")
        numbers, names = [], []
        for s, item in enumerate(segments):
            if SEGMENT_NUMBER not in item:
                _refuse(path, f"malformed: item {s} of SegmentSequence has no SegmentNumber (0062,0004)")
            numbers.append(_integer(buf, item[SEGMENT_NUMBER], "SegmentNumber", path, "US"))
            names.append(_text(buf, item[SEGMENT_LABEL]) if SEGMENT_LABEL in item else "")
        if len(set(numbers)) != len(numbers):
            _refuse(path, f"malformed: SegmentSequence repeats a SegmentNumber ({numbers})")
        per_frame = top.get(PER_FRAME_GROUPS, [])
        if len(per_frame) != n_frames:
            _refuse(path, f"NumberOfFrames {n_frames} and {len(per_frame)} items in PerFrameFunctionalGroupsSequence (5200,9230): one item per frame is expected")
        shared = (top.get(SHARED_GROUPS) or [{}])[0]
        segment_of = np.zeros(n_frames, dtype=np.int32)
        positions, orientations = np.zeros((n_frames, 3)), np.zeros((n_frames, 6))
        spacings, steps = np.full((n_frames, 2), np.nan), np.full(n_frames, np.nan)
        for f, item in enumerate(per_frame):
            position = _group(buf, item, PLANE_POSITION, POSITION, f"ImagePositionPatient of frame {f}", 3, path)
            if position is None:
                _refuse(path, f"frame {f} has no PlanePositionSequence / ImagePositionPatient: without its position the frame cannot be placed")
            number = None
            if item.get(SEGMENT_IDENTIFICATION) and REFERENCED_SEGMENT_NUMBER in item[SEGMENT_IDENTIFICATION][0]:
                number = _integer(buf, item[SEGMENT_IDENTIFICATION][0][REFERENCED_SEGMENT_NUMBER], f"ReferencedSegmentNumber of frame {f}", path, "US")
            if number is None:
                _refuse(path, f"frame {f} has no SegmentIdentificationSequence / ReferencedSegmentNumber: it belongs to no segment")
            if number not in numbers:
                _refuse(path, f"malformed: frame {f} refers to SegmentNumber {number}, SegmentSequence has {numbers}")
            orientation = None
            for source in (item, shared):
                if orientation is None:
                    orientation = _group(buf, source, PLANE_ORIENTATION, ORIENTATION, f"ImageOrientationPatient of frame {f}", 6, path)
            if orientation is None:
                _refuse(path, f"no PlaneOrientationSequence / ImageOrientationPatient in the shared functional groups or in frame {f}: without "
                              "orientation the frames cannot be placed")
            for source in (shared, item):                                  # (a per-frame value overrides the shared one)
                spacing = _group(buf, source, PIXEL_MEASURES, PIXEL_SPACING, f"PixelSpacing of frame {f}", 2, path)
                if spacing is not None:
                    spacings[f] = spacing
                for inner, what in ((SLICE_THICKNESS, "SliceThickness"), (SPACING_BETWEEN, "SpacingBetweenSlices")):   # the latter wins
                    v = _group(buf, source, PIXEL_MEASURES, inner, f"{what} of frame {f}", None, path)
                    if v:
                        steps[f] = v[0]
            segment_of[f], positions[f], orientations[f] = numbers.index(number), position, orientation
        fs = FrameSet(path, names, rows, columns, segment_of, positions, orientations, spacings, steps, None, bool(header_only))
        if header_only:
            return fs
        if PIXEL_DATA not in top:
            _refuse(path, "no PixelData (7FE0,0010)")
        voff, length = top[PIXEL_DATA]
        if length == UNDEFINED:
            _refuse(path, "PixelData of undefined length (encapsulated, i.e. compressed, frames) is outside the path: decompress the file first")
        need = (n_frames * rows * columns + 7) // 8
        have = min(length, size - voff)
        if have < need:
            _refuse(path, f"truncated: {have} bytes of PixelData, {need} expected for {n_frames} frames of {rows} x {columns} bits")
        fs.frame = np.frombuffer(buf, dtype=np.uint8, count=need, offset=voff)
        part.keep = True
        return fs


def resolve(frame_set: FrameSet, roi) -> int:
    """The index of the segment that `roi` (`Data: mask_roi`) names: SegmentLabel, exact and case-insensitive; None takes the only one."""
    return match_name(frame_set.path, frame_set.names, roi, "segment", "labelled")


def select(frame_set: FrameSet, roi=None) -> FrameSet:
    """The FrameSet that holds the one segment `roi` names (see `resolve`): the same frames and PixelData view, with the frames of the
    other segments marked -1 in `segment_of`."""
    i = resolve(frame_set, roi)
    if len(frame_set.names) == 1:
        return frame_set
    return dataclasses.replace(frame_set, names=[frame_set.names[i]], segment_of=np.where(frame_set.segment_of == i, 0, -1).astype(np.int32))


def _on_scan(fs, chosen, shape, m):
    """Slice index per chosen frame when every one of them lies on the scan's lattice (see `to_scan`), else None."""
    x, y, _ = shape
    if (fs.columns, fs.rows) != (x, y):
        return None
    ks = []
    for f in chosen:
        if not np.isfinite(fs.spacings[f]).all():
            return None
        p, r, c = fs.positions[f], fs.orientations[f, :3], fs.orientations[f, 3:]
        corners = (p, p + r * fs.spacings[f, 1] * (x - 1), p + c * fs.spacings[f, 0] * (y - 1))
        idx = [m[:3, :3] @ (q * np.array([-1.0, -1.0, 1.0])) + m[:3, 3] for q in corners]        # LPS -> RAS -> scan voxel index
        k = float(np.floor(idx[0][2] + 0.5))
        want = ((0.0, 0.0, k), (x - 1.0, 0.0, k), (0.0, y - 1.0, k))
        if max(float(np.abs(i - np.asarray(w)).max()) for i, w in zip(idx, want)) > ON_GRID_TOLERANCE:
            return None
        ks.append(int(k))
    return ks


def _arrays(slices, frames, z):
    """refs / slice_first of the C-ABI from the slice of every frame in `frames`."""
    slices, frames = np.asarray(slices, dtype=np.int64), np.asarray(frames, dtype=np.int64)
    order = np.argsort(slices, kind="stable")                # (the file's order within a slice)
    return frames[order].astype(np.int32), np.searchsorted(slices[order], np.arange(z + 1), side="left").astype(np.int32)


def to_scan(frames: FrameSet, scan_shape, scan_affine) -> Placement:
    """Place the frames of one segment (`select`'s result, or a FrameSet of one segment) against a scan of extents `scan_shape` and RAS
    voxel-index -> mm matrix `scan_affine`, in fp64.  Positions are LPS and are flipped to RAS as `dicom.read_series` does.

    On the scan's grid: Rows / Columns equal the scan's and the corners (0,0), (x-1,0), (0,y-1) of every frame map through the inverse
    scan affine to within 1e-3 voxel of (0,0,k), (x-1,0,k), (0,y-1,k) for one integer k per frame.  Frames with k outside 0..z-1 are
    dropped, counted and reported once per file; a segment that leaves nothing on the scan is refused.  The mask is then written
    straight onto the scan's grid with one = 1.

    Otherwise, on a grid of its own: the frames must share one orientation (to 1e-4) and one pixel spacing, stack along their normal
    (in-plane offset <= 1e-3 voxel) at offsets within 0.01 step of whole multiples of the step (SpacingBetweenSlices, else
    SliceThickness, else the smallest positive gap); anything else is refused with the frame named.  The volume is the stack from the
    first to the last occupied position plus one empty slice on either side, its affine formed as `dicom._geometry` forms a series',
    unpacked with one = 255 for `mmnn_resample_mask`."""
    fs = select(frames, None)
    path, name = fs.path, fs.names[0]
    x, y, z = (int(v) for v in scan_shape)
    chosen = np.flatnonzero(fs.segment_of == 0)
    if chosen.size == 0:
        raise ConfigurationError(f"{path}: segment {name!r} has no frames: it leaves nothing on the scan")
    if scan_affine is None:
        raise ConfigurationError(f"{path}: the scan has no geometry (position / orientation), so the frames of the segmentation cannot be placed against it")
    scan_affine = np.asarray(scan_affine, dtype=np.float64)
    ks = _on_scan(fs, chosen, (x, y, z), np.linalg.inv(scan_affine))
    if ks is not None:
        inside = [0 <= k < z for k in ks]
        dropped = len(ks) - sum(inside)
        if dropped and path not in _warned:
            _warned.add(path)
            logger.warning("%s, segment %r: dropped %d frame(s): slice outside the scan", path, name, dropped)
        if not any(inside):
            raise ConfigurationError(f"{path}: segment {name!r} leaves nothing on the scan's {z} slices (dropped: {dropped} frame(s) outside the scan)")
        refs, slice_first = _arrays([k for k, i in zip(ks, inside) if i], [f for f, i in zip(chosen, inside) if i], z)
        return Placement((x, y, z), scan_affine, refs, slice_first, 1, True, dropped, path)
    # ---- a stack of its own
    first = int(chosen[0])
    ori = fs.orientations[first]
    r, c = ori[:3], ori[3:]
    n = np.cross(r, c)
    if np.linalg.norm(n) < 1e-6:
        _refuse(path, f"ImageOrientationPatient {tuple(ori)} of frame {first} spans no plane")
    spacing = fs.spacings[first]
    if not np.isfinite(spacing).all() or spacing.min() <= 0.0:
        _refuse(path, f"frame {first} has no PixelSpacing (PixelMeasuresSequence), and the frames do not lie on the scan's grid: without it the "
                      "segmentation's own grid is unknown")
    for f in chosen[1:]:
        if np.abs(fs.orientations[f] - ori).max() > ORIENTATION_TOLERANCE:
            _refuse(path, f"frames {first} and {int(f)} of segment {name!r} differ in ImageOrientationPatient ({tuple(ori)} and {tuple(fs.orientations[f])})")
        if not np.abs(fs.spacings[f] - spacing).max() <= 1e-6 * spacing.max():
            _refuse(path, f"frames {first} and {int(f)} of segment {name!r} differ in PixelSpacing ({tuple(spacing)} and {tuple(fs.spacings[f])})")
    along = fs.positions[chosen] @ n
    base = int(chosen[int(np.argmin(along))])
    p0 = fs.positions[base]
    for f in chosen:
        d = fs.positions[f] - p0
        off = max(abs(float(d @ r)) / spacing[1], abs(float(d @ c)) / spacing[0])
        if off > IN_PLANE_TOLERANCE:
            _refuse(path, f"frame {int(f)} of segment {name!r} is shifted {off:.3g} voxel in its plane against frame {base}: the frames do not stack along their normal")
    rel = along - along.min()
    declared = fs.steps[chosen]
    declared = declared[np.isfinite(declared) & (declared > 0.0)]
    gaps = np.diff(np.unique(rel))
    gaps = gaps[gaps > 1e-6]
    step = float(declared[0]) if declared.size else (float(gaps.min()) if gaps.size else 1.0)
    q = rel / step
    index = np.floor(q + 0.5)
    for f, qi, ii in zip(chosen, q, index):
        if abs(qi - ii) > STEP_TOLERANCE:
            _refuse(path, f"frame {int(f)} of segment {name!r} lies {qi:.4g} steps of {step:.6g} mm above frame {base} along the normal, no whole "
                          "number: the frames form no regular stack")
    top = int(index.max())
    last = int(chosen[int(np.argmax(along))])
    v = (fs.positions[last] - p0) / top if top > 0 else n * step
    lps = np.eye(4, dtype=np.float64)
    lps[:3, 0], lps[:3, 1], lps[:3, 2], lps[:3, 3] = r * spacing[1], c * spacing[0], v, p0 - v        # (slice 0 is the empty one below the first)
    refs, slice_first = _arrays(index.astype(np.int64) + 1, chosen, top + 3)
    return Placement((int(fs.columns), int(fs.rows), top + 3), lps_to_ras(lps), refs, slice_first, 255, False, 0, path)
