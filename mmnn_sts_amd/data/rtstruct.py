"""A minimal RT Structure Set reader (numpy only, on `dicom.py`'s file opener, nested data-set walk and value helpers): the planar contours
of the regions of interest a contouring workstation exports, and their mapping onto a scan's voxel grid for the device rasteriser
(`mmnn_sts_amd.data.ingest.rasterize_contours`, `mmnn_rasterize_contours`).  The host parses the file and moves the contour points into
the scan's index space; it fills no voxel.

An RTSTRUCT file is a part-10 file of SOP class 1.2.840.10008.5.1.4.1.1.481.3 whose data set nests sequences, which `dicom.read_file`
skips and `dicom.walk` descends into (`ENTERED`, keeping the elements in `KEPT`):

    StructureSetROISequence (3006,0020)   per ROI: ROINumber (3006,0022), ReferencedFrameOfReferenceUID (3006,0024), ROIName (3006,0026)
    ROIContourSequence (3006,0039)        per ROI: ReferencedROINumber (3006,0084) and ContourSequence (3006,0040), per contour:
                                          ContourGeometricType (3006,0042), NumberOfContourPoints (3006,0046), ContourData (3006,0050)

in explicit or implicit VR little endian, with sequences and items of defined or undefined length; in implicit VR the sequences to enter
are recognised by tag.  ContourData is a DS string of x\\y\\z triplets in patient millimetres, LPS.  Only CLOSED_PLANAR contours are kept;
the others are counted.  The refusals of `dicom.py` hold: compressed, big endian and deflated syntaxes, truncated elements, nesting
beyond `MAX_DEPTH`.  DICOM SEG is another object: `read` refuses it; `seg.py` reads it.

    read(path, header_only=False)                 -> ContourSet: ROI names in file order and, per ROI, its (n, 3) float64 contours
    select(contour_set, roi)                      -> the ContourSet of one ROI (name match exact, case-insensitive; None: the only one)
    to_scan_index(contours, shape, affine)        -> (points, contours, slice_first, dropped): what `mmnn_rasterize_contours` takes

Parity with the rasterisation of SimpleITK / plastimatch / rt-utils is unpinned: none is installed where this was written.  The path is
pinned to the standard's element layout, to the even-odd rule stated above `mmnn_rasterize_contours` in the header, and to the NIfTI
twin (`synth_dicom.from_nifti_tree(..., mask_format="rtstruct")` must give the same device batch as the NIfTI tree, bit for bit).
"""
import logging
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from ..exceptions.exceptions import ConfigurationError
from .dicom import _check_syntax, _integer, _refuse, _text, match_name, part10, walk

logger = logging.getLogger(__name__)

RT_STRUCTURE_SET_STORAGE = "1.2.840.10008.5.1.4.1.1.481.3"
SOP_CLASS_UID = (0x0008, 0x0016)
STRUCTURE_SET_ROI_SEQUENCE, ROI_CONTOUR_SEQUENCE, CONTOUR_SEQUENCE = (0x3006, 0x0020), (0x3006, 0x0039), (0x3006, 0x0040)
ROI_NUMBER, FRAME_OF_REFERENCE_UID, ROI_NAME, REFERENCED_ROI_NUMBER = (0x3006, 0x0022), (0x3006, 0x0024), (0x3006, 0x0026), (0x3006, 0x0084)
CONTOUR_GEOMETRIC_TYPE, NUMBER_OF_CONTOUR_POINTS, CONTOUR_DATA = (0x3006, 0x0042), (0x3006, 0x0046), (0x3006, 0x0050)
ENTERED = frozenset((STRUCTURE_SET_ROI_SEQUENCE, ROI_CONTOUR_SEQUENCE, CONTOUR_SEQUENCE))      # the sequences the walk descends into
KEPT = frozenset((SOP_CLASS_UID, ROI_NUMBER, FRAME_OF_REFERENCE_UID, ROI_NAME, REFERENCED_ROI_NUMBER, CONTOUR_GEOMETRIC_TYPE,
                  NUMBER_OF_CONTOUR_POINTS, CONTOUR_DATA))
MAX_SLICE_SPREAD = 0.25                      # slices: a planar contour drawn on this scan's slice planes stays far below it
_warned = set()                              # files whose dropped contours have been reported


@dataclass
class ContourSet:
    """The regions of interest of one file.  `names`: ROIName in file order; `contours[r]`: the CLOSED_PLANAR contours of ROI r of at
    least 3 points, each an (n, 3) float64 array of LPS millimetres (empty lists with header_only); `dropped[r]`: what was left out of
    ROI r, by reason; `frames[r]`: its ReferencedFrameOfReferenceUID or None."""
    path: str
    names: List[str]
    contours: List[List[np.ndarray]] = field(default_factory=list)
    dropped: List[Dict[str, int]] = field(default_factory=list)
    frames: List[Optional[str]] = field(default_factory=list)
    header_only: bool = False


def _contour(buf, item, path, roi_name, index):
    """(points or None, reason it was dropped or None) of one item of a ContourSequence."""
    kind = _text(buf, item[CONTOUR_GEOMETRIC_TYPE]).upper() if CONTOUR_GEOMETRIC_TYPE in item else ""
    what = f"contour {index} of ROI {roi_name!r}"
    text = _text(buf, item[CONTOUR_DATA]) if CONTOUR_DATA in item else ""
    try:
        values = np.array(text.split("\\"), dtype=np.float64) if text else np.zeros(0, dtype=np.float64)      # one conversion per contour
    except ValueError:
        _refuse(path, f"malformed: ContourData of {what} holds something that is no decimal string ({text[:32]!r}...)")
    if values.size % 3:
        _refuse(path, f"malformed: ContourData of {what} holds {values.size} numbers, no whole number of x\\y\\z triplets")
    if NUMBER_OF_CONTOUR_POINTS in item:
        declared = _integer(buf, item[NUMBER_OF_CONTOUR_POINTS], f"NumberOfContourPoints of {what}", path)
        if declared != values.size // 3:
            _refuse(path, f"malformed: {what} declares NumberOfContourPoints {declared} and its ContourData holds {values.size // 3} points")
    if kind != "CLOSED_PLANAR":
        return None, kind or "no ContourGeometricType"
    if not np.isfinite(values).all():
        _refuse(path, f"malformed: ContourData of {what} holds a non-finite number")
    if values.size < 9:
        return None, "fewer than 3 points"
    return values.reshape(-1, 3), None


def read(path, header_only=False) -> ContourSet:
    """Parse an RTSTRUCT file.  With `header_only` the walk stops behind StructureSetROISequence: the ROI names alone."""
    with part10(path) as f:
        path, buf = f.path, f.buf
        explicit, _ = _check_syntax(f.syntax, path)
        top, _ = walk(buf, f.off, f.size, explicit, path, KEPT, ENTERED, stop_after=STRUCTURE_SET_ROI_SEQUENCE if header_only else None)
        sop = _text(buf, top[SOP_CLASS_UID]) if SOP_CLASS_UID in top else None
        if sop != RT_STRUCTURE_SET_STORAGE:
            _refuse(path, f"SOPClassUID {sop} is not RT Structure Set Storage ({RT_STRUCTURE_SET_STORAGE})"
                          + (": DICOM SEG is outside the path" if sop == "1.2.840.10008.5.1.4.1.1.66.4" else ""))
        rois = top.get(STRUCTURE_SET_ROI_SEQUENCE, [])
        if not rois:
            _refuse(path, "no StructureSetROISequence (3006,0020): the structure set names no region of interest")
        numbers, names, frames = [], [], []
        for r, item in enumerate(rois):
            if ROI_NUMBER not in item:
                _refuse(path, f"malformed: item {r} of StructureSetROISequence has no ROINumber (3006,0022)")
            numbers.append(_integer(buf, item[ROI_NUMBER], "ROINumber", path))
            names.append(_text(buf, item[ROI_NAME]) if ROI_NAME in item else "")
            frames.append((_text(buf, item[FRAME_OF_REFERENCE_UID]) or None) if FRAME_OF_REFERENCE_UID in item else None)
        if len(set(numbers)) != len(numbers):
            _refuse(path, f"malformed: StructureSetROISequence repeats an ROINumber ({numbers})")
        cs = ContourSet(path, names, [[] for _ in names], [{} for _ in names], frames, bool(header_only))
        if header_only:
            return cs
        for item in top.get(ROI_CONTOUR_SEQUENCE, []):
            if REFERENCED_ROI_NUMBER not in item:
                _refuse(path, "malformed: an item of ROIContourSequence has no ReferencedROINumber (3006,0084)")
            number = _integer(buf, item[REFERENCED_ROI_NUMBER], "ReferencedROINumber", path)
            if number not in numbers:
                _refuse(path, f"malformed: ROIContourSequence refers to ROINumber {number}, StructureSetROISequence has {numbers}")
            r = numbers.index(number)
            for index, contour in enumerate(item.get(CONTOUR_SEQUENCE, [])):
                points, reason = _contour(buf, contour, path, names[r], index)
                if points is None:
                    cs.dropped[r][reason] = cs.dropped[r].get(reason, 0) + 1
                else:
                    cs.contours[r].append(points)
        return cs


def resolve(contour_set: ContourSet, roi) -> int:
    """The index of the ROI that `roi` (`Data: mask_roi`) names: exact and case-insensitive; None takes the only ROI."""
    return match_name(contour_set.path, contour_set.names, roi, "ROI", "named")


def select(contour_set: ContourSet, roi=None) -> ContourSet:
    """The ContourSet that holds the one ROI `roi` names (see `resolve`)."""
    i = resolve(contour_set, roi)
    if len(contour_set.names) == 1:
        return contour_set
    return ContourSet(contour_set.path, [contour_set.names[i]], [contour_set.contours[i]] if contour_set.contours else [],
                      [contour_set.dropped[i]] if contour_set.dropped else [], [contour_set.frames[i]] if contour_set.frames else [],
                      contour_set.header_only)


def to_scan_index(contours, scan_shape, scan_affine):
    """Contours in LPS millimetres -> what `mmnn_rasterize_contours` takes for a scan of extents `scan_shape` and RAS voxel-index -> mm
    matrix `scan_affine`: (points (P, 2) float64 = (i, j) in continuous voxel index coordinates, contours (C, 2) int32 = (first point,
    point count) sorted by slice, slice_first (z + 1) int32, dropped {reason: count}).  `contours`: a ContourSet of one ROI (what `select`
    returns) or a list of (n, 3) arrays.  Each point is flipped to RAS and taken through the inverse of
    the affine; a contour belongs to slice round(mean k).  Refused: a contour that spreads more than 0.25 slice along k (it was not
    drawn on this scan's slice planes), an ROI of which nothing is left.  Dropped and counted: contours of other geometric types and of
    fewer than 3 points (by `read`), contours whose slice lies outside the scan; one warning per file says so."""
    path, name, dropped = "contours", None, {}
    if isinstance(contours, ContourSet):
        cs = select(contours, None)
        if cs.header_only:
            raise ValueError(f"to_scan_index: {cs.path} was read with header_only: it holds no contours")
        path, name, dropped, contours = cs.path, cs.names[0], dict(cs.dropped[0]), cs.contours[0]
    x, y, z = (int(v) for v in scan_shape)
    if scan_affine is None:
        raise ConfigurationError(f"{path}: the scan has no geometry (position / orientation), so its contours cannot be placed on its grid")
    m = np.linalg.inv(np.asarray(scan_affine, dtype=np.float64))
    placed = []
    for index, pts in enumerate(contours):
        pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f"to_scan_index: contour {index} has shape {pts.shape}, (n, 3) expected")
        if len(pts) < 3:
            dropped["fewer than 3 points"] = dropped.get("fewer than 3 points", 0) + 1
            continue
        rx, ry, rz = -pts[:, 0], -pts[:, 1], pts[:, 2]            # LPS -> RAS
        i, j, k = (m[r, 0] * rx + m[r, 1] * ry + m[r, 2] * rz + m[r, 3] for r in range(3))
        spread = float(k.max() - k.min())
        if spread > MAX_SLICE_SPREAD:
            raise ConfigurationError(f"{path}: contour {index}{'' if name is None else f' of ROI {name!r}'} spreads {spread:.3g} slices along the scan's "
                                     f"slice axis (more than {MAX_SLICE_SPREAD}): it was not drawn on this scan's slice planes (another series, an "
                                     "oblique reformat).  Export the structure set on the scan it is used with")
        s = int(np.floor(float(k.mean()) + 0.5))
        if not 0 <= s < z:
            dropped["slice outside the scan"] = dropped.get("slice outside the scan", 0) + 1
            continue
        placed.append((s, np.stack([i, j], axis=1)))
    if dropped and path not in _warned:
        _warned.add(path)
        logger.warning("%s%s: dropped %s", path, "" if name is None else f", ROI {name!r}", ", ".join(f"{n} contour(s): {r}" for r, n in sorted(dropped.items())))
    if not placed:
        raise ConfigurationError(f"{path}: {'the contours leave' if name is None else f'ROI {name!r} leaves'} nothing on the scan's {z} slices"
                                 + (f" (dropped: {dropped})" if dropped else " (it has no contours)"))
    placed.sort(key=lambda t: t[0])                             # (stable: the file's order within a slice)
    counts = np.asarray([len(p) for _, p in placed], dtype=np.int64)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    if int(counts.sum()) >= 2 ** 31:
        raise ConfigurationError(f"{path}: {int(counts.sum())} contour points")
    slices = np.asarray([s for s, _ in placed], dtype=np.int64)
    slice_first = np.searchsorted(slices, np.arange(z + 1), side="left").astype(np.int32)
    return (np.ascontiguousarray(np.concatenate([p for _, p in placed], axis=0)), np.stack([firsts, counts], axis=1).astype(np.int32), slice_first, dropped)
