"""A minimal DICOM reader for uncompressed, RLE Lossless and JPEG Lossless single-frame series (numpy, mmap and struct only; pydicom /
GDCM / SimpleITK are not dependencies): a directory of slice files -> the raw voxel bytes (or the RLE / JPEG fragments), the per-slice
rescale pairs and the voxel-index -> mm matrix that the device ingest takes (`mmnn_sts_amd.data.ingest.decode_series`).  The host opens
files, parses headers and copies bytes; it never touches a voxel value -- expanding the PackBits runs of an RLE series
(`mmnn_rle_expand`), Huffman decoding and prediction of a JPEG Lossless series (`mmnn_jpegll_decode`), unpacking the stored bits, sign
extension and per-slice rescaling (`mmnn_decode_slices`) run on the device.

Pinned to the published standard's element layout (PS3.5 / PS3.10): the 128-byte preamble and `DICM`; the file meta group (0002,xxxx),
always explicit VR little endian; then the data set in the VR mode TransferSyntaxUID (0002,0010) names.  An explicit-VR element is
tag (2 + 2 bytes), VR (2 characters) and a 2-byte length, or -- for OB OD OF OL OV OW SQ SV UC UN UR UT UV -- 2 reserved bytes and a 4-byte
length; an implicit-VR element is tag and a 4-byte length.  A length of FFFFFFFF is "undefined": the value is a sequence of items
(FFFE,E000), each of defined or undefined length, closed by (FFFE,E00D) / (FFFE,E0DD).  Parity with GDCM / SimpleITK (what upstream's
`loadImage` / `loadMask` read through, data/utils.py:16-37) is unpinned: neither is installed where this was written.  What it is
pinned to instead is that layout and the NIfTI twin: `synth_dicom.from_nifti_tree` turns a NIfTI tree into a DICOM one, and the two
must give the same device batch bit for bit.

Accepted: implicit VR little endian (1.2.840.10008.1.2), explicit VR little endian (1.2.840.10008.1.2.1) and RLE Lossless
(1.2.840.10008.1.2.5, PS3.5 Annex G), SamplesPerPixel 1, one frame per file, BitsAllocated 8 / 16 / 32.  An RLE file's data set is
explicit VR little endian and its PixelData is encapsulated (PS3.5 A.4): OB of undefined length holding the Basic Offset Table item
(its content is ignored), one fragment item for the one frame, and the sequence delimiter.  The host reads the fragment's 64-byte
header -- 16 little-endian uint32: the segment count (BitsAllocated / 8), then 15 offsets from the start of the header -- checks it and
reads nothing behind it: `encoding` is 'rle', `frame` the whole fragment and `segments` its (offset, length) pairs.  JPEG Lossless,
Non-Hierarchical, First-Order Prediction (1.2.840.10008.1.2.4.70; T.81 Annex H, process 14 with selection value 1) and its sibling
1.2.840.10008.1.2.4.57 when its scan header selects predictor 1 are encapsulated alike.  Of that fragment the host reads the marker
segments in front of the entropy-coded data -- SOI, APPn / COM (skipped), DHT, SOF3, SOS -- and no entropy-coded byte: it does not
un-stuff and does not look for EOI.  `encoding` is 'jpeg-lossless', `frame` the whole fragment and `jpeg` a `JpegScan`: the precision,
the Huffman table SOS selects and where the data behind SOS lies.  Refused, with the file named: big endian, deflated, every other
encapsulated (compressed) syntax -- JPEG baseline / extended, JPEG-LS, JPEG 2000 among them --, predictors 2-7, restart intervals,
several fragments, multi-frame and enhanced objects, colour, float / double pixel data, and a series that mixes encodings.  A mask may also be an RT Structure Set: that file is read by
`rtstruct.py`, or a BINARY DICOM Segmentation object, read by `seg.py`.  What the three readers share lives here once: `part10` (the
one place a file is mapped), `walk` (the nested data-set walk that descends into the sequences `read_file` skips), the value helpers
`_text` / `_integer` / `_floats`, `match_name` behind both `resolve`s and `lps_to_ras`.  `read_file` itself keeps refusing every
multi-frame file.

`read_series(directory)` sorts the slices by position along the normal of ImageOrientationPatient -- file names and InstanceNumber play
no part -- and forms the affine in RAS, the convention of `NiftiImage.affine`, so `nifti.index_map`, `KeptVolume.affine` and the
`--scan_space` writer work on a series as they do on a NIfTI file.  Voxel index (i, j, k) is (column, row, slice).
"""
import logging
import mmap
import os
import struct
from contextlib import contextmanager
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import List, Optional, Tuple

import numpy as np

from ..exceptions.exceptions import ConfigurationError

logger = logging.getLogger(__name__)

IMPLICIT_LE = "1.2.840.10008.1.2"
EXPLICIT_LE = "1.2.840.10008.1.2.1"
RLE_LOSSLESS = "1.2.840.10008.1.2.5"
JPEG_LOSSLESS, JPEG_LOSSLESS_SV1 = "1.2.840.10008.1.2.4.57", "1.2.840.10008.1.2.4.70"
NATIVE, RLE, JPEGLL = "native", "rle", "jpeg-lossless"       # DicomFile.encoding
_ENCODING_NAME = {RLE: "RLE lossless", JPEGLL: "JPEG lossless"}
RLE_HEADER_BYTES = 64                        # 16 uint32: the segment count and 15 offsets
_REFUSED_SYNTAX = {"1.2.840.10008.1.2.2": "explicit VR big endian", "1.2.840.10008.1.2.1.99": "deflated explicit VR little endian"}
LONG_VRS = frozenset(("OB", "OD", "OF", "OL", "OV", "OW", "SQ", "SV", "UC", "UN", "UR", "UT", "UV"))
UNDEFINED = 0xFFFFFFFF
ITEM, ITEM_END, SEQUENCE_END = (0xFFFE, 0xE000), (0xFFFE, 0xE00D), (0xFFFE, 0xE0DD)
PIXEL_DATA, FLOAT_PIXEL_DATA, DOUBLE_PIXEL_DATA = (0x7FE0, 0x0010), (0x7FE0, 0x0008), (0x7FE0, 0x0009)
MAX_DEPTH = 32                               # nesting of undefined-length sequences followed before the file is called malformed

# tag -> (field, VR); the VR is what an implicit-VR file does not say
KEPT = {
    (0x0008, 0x0016): ("sop_class_uid", "UI"), (0x0018, 0x0050): ("slice_thickness", "DS"), (0x0018, 0x0088): ("spacing_between_slices", "DS"),
    (0x0020, 0x000E): ("series_uid", "UI"), (0x0020, 0x0013): ("instance_number", "IS"), (0x0020, 0x0032): ("position", "DS"),
    (0x0020, 0x0037): ("orientation", "DS"), (0x0028, 0x0002): ("samples_per_pixel", "US"), (0x0028, 0x0008): ("number_of_frames", "IS"),
    (0x0028, 0x0010): ("rows", "US"), (0x0028, 0x0011): ("columns", "US"), (0x0028, 0x0030): ("pixel_spacing", "DS"),
    (0x0028, 0x0100): ("bits_allocated", "US"), (0x0028, 0x0101): ("bits_stored", "US"), (0x0028, 0x0102): ("high_bit", "US"),
    (0x0028, 0x0103): ("pixel_representation", "US"), (0x0028, 0x1052): ("inter", "DS"), (0x0028, 0x1053): ("slope", "DS"),
}
_ARITY = {"position": 3, "orientation": 6, "pixel_spacing": 2}


class NotDicomError(ConfigurationError):
    """The file has no `DICM` magic (read_series skips such files)."""


@dataclass
class JpegScan:
    """What the marker segments of a JPEG Lossless fragment say: `precision` P of SOF3; `lines`, `samples` per line; `bits`, the 16
    BITS counts of the Huffman table SOS selects, and `huffval`, its values in code order (at most 17, each in 0..16); `offset`,
    `length`: the bytes behind the SOS segment, relative to the fragment (entropy-coded data, EOI and whatever follows)."""
    precision: int
    lines: int
    samples: int
    bits: np.ndarray
    huffval: np.ndarray
    offset: int
    length: int


@dataclass
class DicomFile:
    """The kept elements of one file.  Absent elements are None, except slope / inter (1 / 0)."""
    path: str
    transfer_syntax: str
    rows: Optional[int] = None
    columns: Optional[int] = None
    samples_per_pixel: Optional[int] = None
    bits_allocated: Optional[int] = None
    bits_stored: Optional[int] = None
    high_bit: Optional[int] = None
    pixel_representation: Optional[int] = None
    slope: float = 1.0
    inter: float = 0.0
    pixel_spacing: Optional[Tuple[float, float]] = None
    position: Optional[Tuple[float, float, float]] = None
    orientation: Optional[Tuple[float, ...]] = None
    slice_thickness: Optional[float] = None
    spacing_between_slices: Optional[float] = None
    series_uid: Optional[str] = None
    instance_number: Optional[float] = None
    number_of_frames: Optional[float] = None
    sop_class_uid: Optional[str] = None
    pixel_offset: Optional[int] = None       # byte offset of the PixelData value in the file; None: the file has no PixelData
    pixel_length: Optional[int] = None       # its declared length
    frame: Optional[np.ndarray] = None       # uint8 view of the rows * columns * bits_allocated / 8 voxel bytes, or, 'rle' and
                                             # 'jpeg-lossless', of the whole fragment, header included (None with header_only)
    encoding: str = NATIVE                   # NATIVE, RLE: `frame` holds PackBits segments, or JPEGLL: a JPEG Lossless stream
    segments: Optional[np.ndarray] = None    # 'rle': (bits_allocated / 8, 2) int64, byte offset into the fragment and byte length
    jpeg: Optional[JpegScan] = None          # 'jpeg-lossless'

    @property
    def has_image(self):
        return self.rows is not None and self.columns is not None and self.pixel_offset is not None


def _refuse(path, reason):
    raise ConfigurationError(f"{path}: {reason}")


def _need(buf, off, count, path):
    if off + count > len(buf):
        _refuse(path, f"malformed: an element header at byte {off} runs past the end of the file ({len(buf)} bytes)")


def _element(buf, off, explicit, path):
    """(tag, VR or None, length, offset of the value) of the element at `off`.  Item tags carry no VR in either mode."""
    _need(buf, off, 8, path)
    tag = struct.unpack_from("<HH", buf, off)
    if not explicit or tag[0] == 0xFFFE:
        return tag, None, struct.unpack_from("<I", buf, off + 4)[0], off + 8
    vr = bytes(buf[off + 4:off + 6]).decode("latin-1")
    if vr in LONG_VRS:
        _need(buf, off, 12, path)
        return tag, vr, struct.unpack_from("<I", buf, off + 8)[0], off + 12
    return tag, vr, struct.unpack_from("<H", buf, off + 6)[0], off + 8


def _skip_sequence(buf, off, explicit, path, depth=0):
    """`off`: the first item of a sequence of undefined length; returns the offset behind its delimiter (FFFE,E0DD)."""
    if depth > MAX_DEPTH:
        _refuse(path, f"malformed: sequences nested deeper than {MAX_DEPTH}")
    while True:
        tag, _, length, voff = _element(buf, off, explicit, path)
        if tag == SEQUENCE_END:
            return voff
        if tag != ITEM:
            _refuse(path, f"malformed: ({tag[0]:04X},{tag[1]:04X}) at byte {off} where an item of a sequence was expected")
        off = voff + length if length != UNDEFINED else _skip_item(buf, voff, explicit, path, depth)


def _skip_item(buf, off, explicit, path, depth):
    """`off`: the first element of an item of undefined length; returns the offset behind its delimiter (FFFE,E00D)."""
    while True:
        tag, vr, length, voff = _element(buf, off, explicit, path)
        if tag == ITEM_END:
            return voff
        if length == UNDEFINED:              # a nested sequence; the content of an undefined-length UN is implicit VR (PS3.5 6.2.2)
            off = _skip_sequence(buf, voff, explicit and vr != "UN", path, depth + 1)
        else:
            off = voff + length


def _numbers(raw):
    """A DS / IS value: split on the backslash, stripped of spaces and NULs, as Python floats (an empty value: no numbers)."""
    return [float(p) for p in (q.strip(" \0") for q in raw.decode("latin-1").split("\\")) if p]


def _value(buf, name, vr, voff, length, path):
    raw = bytes(buf[voff:voff + length])
    try:
        if vr == "US":
            return struct.unpack_from("<H", raw, 0)[0] if length >= 2 else None
        if vr == "UI":
            return raw.decode("latin-1").strip(" \0") or None
        v = _numbers(raw)
    except (ValueError, struct.error):
        _refuse(path, f"malformed: {name} holds {raw[:32]!r}")
    if name in _ARITY:
        if not v:
            return None
        if len(v) != _ARITY[name]:
            _refuse(path, f"malformed: {name} holds {len(v)} values, {_ARITY[name]} expected")
        return tuple(v)
    return v[0] if v else None


def _text(buf, value):
    voff, length = value
    return bytes(buf[voff:voff + length]).decode("latin-1").strip(" \0")


def _integer(buf, value, what, path, vr="IS"):
    """The integer of an element found by `walk`: a binary US, else a decimal string (IS, DS)."""
    voff, length = value
    if vr == "US":
        if length < 2:
            _refuse(path, f"malformed: {what} is empty")
        return struct.unpack_from("<H", buf, voff)[0]
    text = _text(buf, value)
    try:
        return int(float(text))
    except ValueError:
        _refuse(path, f"malformed: {what} holds {text[:32]!r}")


def _floats(buf, value, what, count, path):
    """The finite numbers of a DS element found by `walk`, `count` of them (None: any number)."""
    voff, length = value
    raw = bytes(buf[voff:voff + length])
    try:
        v = _numbers(raw)
    except ValueError:
        _refuse(path, f"malformed: {what} holds {raw[:32]!r}")
    if count is not None and len(v) != count:
        _refuse(path, f"malformed: {what} holds {len(v)} values, {count} expected")
    if not np.isfinite(v).all():
        _refuse(path, f"malformed: {what} holds a non-finite number")
    return v


def walk(buf, off, end, explicit, path, kept, entered, depth=0, stop_after=None, pixel_data=False):
    """The elements of one data set (the file's, or an item's) from `off`: {tag: (value offset, length)} for the tags in `kept` and
    {tag: [item, ...]} for the sequences in `entered`, which it descends into (in implicit VR they are recognised by tag).  `end`:
    where the data set ends, or None for an item of undefined length (closed by its delimiter).  Where the file's own data set stops:
    behind tag `stop_after`, or, with `pixel_data`, at PixelData, whose (value offset, declared length) is recorded without looking
    at the value.  Returns (elements, offset behind the data set)."""
    if depth > MAX_DEPTH:
        _refuse(path, f"malformed: sequences nested deeper than {MAX_DEPTH}")
    found = {}
    while end is None or off < end:
        tag, vr, length, voff = _element(buf, off, explicit, path)
        if tag == ITEM_END and end is None:
            return found, voff
        if tag[0] == 0xFFFE:
            _refuse(path, f"malformed: item tag ({tag[0]:04X},{tag[1]:04X}) at byte {off} outside a sequence")
        if stop_after is not None and tag > stop_after:
            break
        if pixel_data and tag >= PIXEL_DATA:
            if tag == PIXEL_DATA:
                found[tag] = (voff, length)
            break
        inner_explicit = explicit and vr != "UN"      # the content of a UN element of undefined length is implicit VR (PS3.5 6.2.2)
        if tag in entered and (vr in (None, "SQ") or (vr == "UN" and length == UNDEFINED)):
            found[tag], off = _items(buf, voff, length, inner_explicit, path, kept, entered, depth + 1)
            continue
        if length == UNDEFINED:
            off = _skip_sequence(buf, voff, inner_explicit, path, depth)
            continue
        limit = len(buf) if end is None else end
        if voff + length > limit:
            _refuse(path, f"malformed: element ({tag[0]:04X},{tag[1]:04X}) at byte {off} declares {length} bytes, {limit - voff} are left")
        if tag in kept:
            found[tag] = (voff, length)
        off = voff + length
    return found, off


def _items(buf, off, length, explicit, path, kept, entered, depth):
    """The items of a sequence whose value starts at `off`: ([elements of each item], offset behind the sequence)."""
    end = None if length == UNDEFINED else off + length
    if end is not None and end > len(buf):
        _refuse(path, f"malformed: a sequence at byte {off} declares {length} bytes, {len(buf) - off} are left")
    items = []
    while end is None or off < end:
        tag, _, ilen, voff = _element(buf, off, explicit, path)
        if tag == SEQUENCE_END and end is None:
            return items, voff
        if tag != ITEM:
            _refuse(path, f"malformed: ({tag[0]:04X},{tag[1]:04X}) at byte {off} where an item of a sequence was expected")
        if ilen == UNDEFINED:
            found, off = walk(buf, voff, None, explicit, path, kept, entered, depth)
        else:
            limit = len(buf) if end is None else end
            if voff + ilen > limit:
                _refuse(path, f"malformed: an item at byte {off} declares {ilen} bytes, {limit - voff} are left")
            found, off = walk(buf, voff, voff + ilen, explicit, path, kept, entered, depth)
        items.append(found)
    return items, off


def match_name(path, names, roi, noun, verb):
    """The index into `names` of the one that `roi` (`Data: mask_roi`) names: exact and case-insensitive; None takes the only one.
    `noun`, `verb`: what the file calls them ("ROI" / "named", "segment" / "labelled")."""
    listed = ", ".join(repr(n) for n in names)
    if roi is None:
        if len(names) == 1:
            return 0
        raise ConfigurationError(f"{path} holds {len(names)} {noun}s ({listed}): name one with Data.mask_roi")
    hits = [i for i, n in enumerate(names) if n.lower() == str(roi).lower()]
    if not hits:
        raise ConfigurationError(f"{path} has no {noun} {verb} {roi!r}; its {noun}s are {listed}")
    if len(hits) > 1:
        raise ConfigurationError(f"{path} has {len(hits)} {noun}s {verb} {roi!r} ({listed})")
    return hits[0]


def lps_to_ras(lps):
    """A voxel index -> mm matrix in DICOM's LPS as one in RAS, the convention of `NiftiImage.affine`."""
    affine = lps.copy()
    affine[:2, :] *= -1.0
    affine += 0.0                            # (no negative zeros)
    return affine


@contextmanager
def part10(path):
    """Map a part-10 file: yields `f` with `buf` (the mapping), `path`, `size`, `syntax` (TransferSyntaxUID) and `off` (where the data
    set starts).  NotDicomError for a file too short for a preamble or without the magic.  The mapping is closed on the way out unless
    the caller set `f.keep`, as it must when it hands on a zero-copy view of PixelData: the file then stays mapped while the view lives."""
    path = str(path)
    size = os.path.getsize(path)
    if size < 132:
        raise NotDicomError(f"{path}: missing magic: {size} bytes, shorter than a preamble (not a DICOM part-10 file)")
    with open(path, "rb") as fh:
        f = SimpleNamespace(buf=mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ), path=path, size=size, keep=False)
    try:
        f.syntax, f.off = _transfer_syntax(f.buf, path)
        yield f
    finally:
        if not f.keep:
            f.buf.close()


def _transfer_syntax(buf, path):
    """(TransferSyntaxUID, offset of the data set): the file meta group is explicit VR little endian whatever follows it."""
    if len(buf) < 132 or bytes(buf[128:132]) != b"DICM":
        raise NotDicomError(f"{path}: missing magic: no 'DICM' behind a 128-byte preamble (not a DICOM part-10 file)")
    off, syntax = 132, None
    while off + 8 <= len(buf) and struct.unpack_from("<H", buf, off)[0] == 0x0002:
        tag, vr, length, voff = _element(buf, off, True, path)
        if length == UNDEFINED:
            _refuse(path, "malformed: an element of undefined length in the file meta group")
        if tag == (0x0002, 0x0010):
            syntax = bytes(buf[voff:voff + length]).decode("latin-1").strip(" \0")
        off = voff + length
    if not syntax:
        _refuse(path, "no TransferSyntaxUID (0002,0010) in the file meta group")
    return syntax, off


def _check_syntax(syntax, path, jpeg_lossless=False):
    """(explicit VR?, encoding) of an accepted transfer syntax.  `jpeg_lossless`: the caller reads JPEG Lossless frames (`read_file`
    does; an RTSTRUCT or SEG file in that syntax stays refused)."""
    if syntax in (IMPLICIT_LE, EXPLICIT_LE):
        return syntax == EXPLICIT_LE, NATIVE
    if syntax == RLE_LOSSLESS:
        return True, RLE
    if jpeg_lossless and syntax in (JPEG_LOSSLESS, JPEG_LOSSLESS_SV1):
        return True, JPEGLL
    if syntax in _REFUSED_SYNTAX:
        _refuse(path, f"transfer syntax {syntax} ({_REFUSED_SYNTAX[syntax]}) is outside the path: only little endian files, uncompressed, RLE "
                      "lossless or JPEG lossless, are read")
    if syntax.startswith("1.2.840.10008.1.2.4."):
        _refuse(path, f"transfer syntax {syntax} is encapsulated (compressed: JPEG baseline / extended, JPEG-LS, JPEG 2000, MPEG, HEVC; of that "
                      f"family only JPEG Lossless image series, {JPEG_LOSSLESS_SV1} and {JPEG_LOSSLESS} with predictor 1, are read), which is "
                      "outside the path: decompress the series first")
    _refuse(path, f"transfer syntax {syntax} is not supported: only {IMPLICIT_LE}, {EXPLICIT_LE}, {RLE_LOSSLESS}, {JPEG_LOSSLESS_SV1} and "
                  f"{JPEG_LOSSLESS} are read")


def _validate(f: DicomFile, size: int):
    """The refusals of a file that holds an image."""
    path = f.path
    if f.samples_per_pixel is not None and f.samples_per_pixel != 1:
        _refuse(path, f"SamplesPerPixel {f.samples_per_pixel}: colour images are outside the path (1 expected)")
    if f.number_of_frames is not None and f.number_of_frames > 1:
        _refuse(path, f"NumberOfFrames {f.number_of_frames:g}: multi-frame and enhanced DICOM objects are outside the path (one frame per file)")
    if f.rows < 1 or f.columns < 1:
        _refuse(path, f"Rows {f.rows}, Columns {f.columns}")
    if f.bits_allocated not in (8, 16, 32):
        _refuse(path, f"BitsAllocated {f.bits_allocated} is none of 8, 16, 32")
    if f.bits_stored is None:
        f.bits_stored = f.bits_allocated
    if not 1 <= f.bits_stored <= f.bits_allocated:
        _refuse(path, f"BitsStored {f.bits_stored} outside 1..{f.bits_allocated} (BitsAllocated)")
    if f.high_bit is None:
        f.high_bit = f.bits_stored - 1
    if not f.bits_stored - 1 <= f.high_bit <= f.bits_allocated - 1:
        _refuse(path, f"HighBit {f.high_bit} outside {f.bits_stored - 1}..{f.bits_allocated - 1} (BitsStored - 1 .. BitsAllocated - 1)")
    if f.pixel_representation not in (0, 1):
        _refuse(path, f"PixelRepresentation {f.pixel_representation} is neither 0 nor 1")
    if f.encoding != NATIVE:
        if f.pixel_length != UNDEFINED:
            _refuse(path, f"transfer syntax {f.transfer_syntax} ({_ENCODING_NAME[f.encoding]}) is compressed and needs encapsulated PixelData of "
                          f"undefined length; this PixelData declares {f.pixel_length} bytes")
        return None
    if f.pixel_length == UNDEFINED:
        _refuse(path, "PixelData of undefined length (encapsulated, i.e. compressed, frames) is outside the path")
    need = f.rows * f.columns * f.bits_allocated // 8
    have = min(f.pixel_length, size - f.pixel_offset)
    if have < need:
        _refuse(path, f"truncated: {have} bytes of PixelData, {need} expected for {f.rows} x {f.columns} x {f.bits_allocated} bits")
    return need


def _fragment(buf, f: DicomFile, size: int):
    """The one fragment of encapsulated PixelData (PS3.5 A.4) as (offset in the file, length): the Basic Offset Table item, whose
    content is ignored, one fragment item, the sequence delimiter.  No byte of the fragment is read."""
    path = f.path

    def item(off, what):
        if off + 8 > size:
            _refuse(path, f"malformed: PixelData ends at byte {size} without its sequence delimiter (FFFE,E0DD), where {what} was expected")
        tag, _, length, voff = _element(buf, off, True, path)
        if tag == SEQUENCE_END:
            return None, voff
        if tag != ITEM:
            _refuse(path, f"malformed: ({tag[0]:04X},{tag[1]:04X}) at byte {off} inside encapsulated PixelData, where an item (FFFE,E000) was expected")
        if length == UNDEFINED or voff + length > size:
            _refuse(path, f"malformed: {what} at byte {off} declares {'an undefined length' if length == UNDEFINED else f'{length} bytes'}, "
                          f"{size - voff} are left in the file")
        return (voff, length), voff + length

    table, off = item(f.pixel_offset, "the Basic Offset Table")
    if table is None:
        _refuse(path, "malformed: encapsulated PixelData without a Basic Offset Table item")
    fragments = []
    while True:
        fragment, off = item(off, "a fragment or the sequence delimiter")
        if fragment is None:
            break
        fragments.append(fragment)
    if len(fragments) != 1:
        _refuse(path, f"{len(fragments)} fragments in PixelData: one frame per file in exactly one fragment is read")
    return fragments[0]


def _rle_fragment(buf, f: DicomFile, size: int):
    """The one fragment of an RLE file's encapsulated PixelData as (offset in the file, length), its header checked and `f.segments`
    set.  Nothing behind the 64-byte header is read."""
    path = f.path
    at, length = _fragment(buf, f, size)
    if length % 2:
        _refuse(path, f"malformed: an RLE fragment of odd length {length}")
    if length < RLE_HEADER_BYTES:
        _refuse(path, f"malformed: an RLE fragment of {length} bytes, shorter than its {RLE_HEADER_BYTES}-byte header")
    count, *offsets = struct.unpack_from("<16I", buf, at)
    planes = f.bits_allocated // 8
    if count != planes:
        _refuse(path, f"the RLE header counts {count} segments, BitsAllocated {f.bits_allocated} needs {planes}")
    used, spare = offsets[:planes], offsets[planes:]
    if used[0] != RLE_HEADER_BYTES:
        _refuse(path, f"malformed: the first RLE segment starts at byte {used[0]} of its fragment, not behind the {RLE_HEADER_BYTES}-byte header")
    if any(b <= a for a, b in zip(used, used[1:])) or used[-1] > length:
        _refuse(path, f"malformed: RLE segment offsets {used} do not ascend strictly inside a fragment of {length} bytes")
    if any(spare):
        _refuse(path, f"malformed: a non-zero offset behind the {planes} used ones of the RLE header ({spare})")
    f.segments = np.array([[a, b - a] for a, b in zip(used, used[1:] + [length])], dtype=np.int64)
    return at, length


def _huffman_tables(buf, off, end, path, tables):
    """The tables of one DHT segment's body buf[off:end] into `tables`: {identifier: (BITS, HUFFVAL)}, each checked."""
    while off < end:
        if off + 17 > end:
            _refuse(path, "malformed: a Huffman table of the JPEG stream's DHT segment runs past the segment")
        tc, th = buf[off] >> 4, buf[off] & 15
        bits = np.frombuffer(buf, dtype=np.uint8, count=16, offset=off + 1).copy()
        n = int(bits.sum())
        if tc != 0:
            _refuse(path, f"the JPEG stream defines a Huffman table of class {tc}: a lossless stream holds tables of class 0 only")
        if n > 17:
            _refuse(path, f"malformed: a Huffman table of the JPEG stream counts {n} codes (BITS), a lossless table has at most 17")
        if off + 17 + n > end:
            _refuse(path, f"malformed: the {n} values of a Huffman table of the JPEG stream run past its DHT segment")
        values = np.frombuffer(buf, dtype=np.uint8, count=n, offset=off + 17).copy()
        if n and int(values.max()) > 16:
            _refuse(path, f"malformed: a Huffman table of the JPEG stream holds the value {int(values.max())} (HUFFVAL); a lossless category is 0..16")
        if len(set(values.tolist())) != n:
            _refuse(path, f"malformed: a Huffman table of the JPEG stream holds repeated values ({values.tolist()})")
        if sum(int(c) << (16 - l) for l, c in enumerate(bits, 1)) > 1 << 16:
            _refuse(path, f"malformed: a Huffman table of the JPEG stream is over-subscribed (BITS {bits.tolist()}: Kraft sum above 1)")
        tables[th] = (bits, values)
        off += 17 + n


def _jpeg_fragment(buf, f: DicomFile, size: int):
    """The one fragment of a JPEG Lossless file's encapsulated PixelData as (offset in the file, length), the marker segments in front
    of its entropy-coded data checked and `f.jpeg` set.  Nothing behind the SOS segment is read."""
    path = f.path
    if f.bits_allocated == 32:
        _refuse(path, "BitsAllocated 32 in a JPEG lossless file: a JPEG sample has at most 16 bits")
    at, length = _fragment(buf, f, size)
    end = at + length
    if length < 2 or bytes(buf[at:at + 2]) != b"\xff\xd8":
        _refuse(path, "malformed: the JPEG fragment does not start with SOI (FFD8)")
    off, tables, frame = at + 2, {}, None
    while True:
        while off + 1 < end and buf[off] == 0xFF and buf[off + 1] == 0xFF:       # fill bytes in front of a marker
            off += 1
        if off + 4 > end:
            _refuse(path, f"malformed: a marker segment at byte {off - at} of the JPEG fragment runs past its {length} bytes (no SOS found)")
        marker, n = buf[off + 1], struct.unpack_from(">H", buf, off + 2)[0]
        if buf[off] != 0xFF or marker in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= marker <= 0xD7:
            _refuse(path, f"malformed: {bytes(buf[off:off + 2]).hex().upper()} at byte {off - at} of the JPEG fragment, where a marker segment was expected")
        name = f"marker segment FF{marker:02X}"
        if n < 2 or off + 2 + n > end:
            _refuse(path, f"malformed: the {name} at byte {off - at} of the JPEG fragment declares {n} bytes and runs past the fragment's {length}")
        body, behind = off + 4, off + 2 + n
        if marker == 0xC4:
            _huffman_tables(buf, body, behind, path, tables)
        elif marker == 0xC3:
            if n < 8 or n != 8 + 3 * buf[body + 5]:
                _refuse(path, f"malformed: the SOF3 segment of the JPEG stream is {n} bytes long")
            precision, lines, samples, components = struct.unpack_from(">BHHB", buf, body)
            if components != 1:
                _refuse(path, f"the JPEG frame holds {components} components (Nf): colour is outside the path (1 expected)")
            frame = (precision, lines, samples, buf[body + 6])
        elif 0xC0 <= marker <= 0xCF and marker not in (0xC8, 0xCC):
            _refuse(path, f"the JPEG stream's frame header is SOF{marker - 0xC0} (FF{marker:02X}): only SOF3 (FFC3), lossless Huffman, is read; "
                          "JPEG baseline / extended / progressive and arithmetic coding are outside the path")
        elif marker == 0xDD:
            if n != 4:
                _refuse(path, f"malformed: the DRI segment of the JPEG stream is {n} bytes long")
            if struct.unpack_from(">H", buf, body)[0]:
                _refuse(path, f"the JPEG stream sets a restart interval of {struct.unpack_from('>H', buf, body)[0]} (DRI): restart intervals are outside the path")
        elif marker == 0xDC:
            _refuse(path, "the JPEG stream defines its number of lines behind the scan (DNL), which is outside the path")
        elif marker == 0xDA:
            break
        elif not (0xE0 <= marker <= 0xEF or marker == 0xFE):
            _refuse(path, f"the {name} of the JPEG stream is outside the path: SOI, APPn, COM, DHT, SOF3, DRI 0 and SOS are read")
        off = behind
    if frame is None:
        _refuse(path, "malformed: the JPEG stream's SOS comes without a frame header (SOF3) in front of it")
    precision, lines, samples, component = frame
    if n < 6 or n != 6 + 2 * buf[body]:
        _refuse(path, f"malformed: the SOS segment of the JPEG stream is {n} bytes long")
    if buf[body] != 1:
        _refuse(path, f"the JPEG scan holds {buf[body]} components (Ns): 1 expected")
    selected, table, predictor, _, transform = struct.unpack_from(">BBBBB", buf, body + 1)
    if selected != component:
        _refuse(path, f"malformed: the JPEG scan selects component {selected}, the frame defines {component}")
    if not 1 <= predictor <= 7:
        _refuse(path, f"malformed: the JPEG scan selects predictor {predictor} (Ss); a lossless scan has 1..7")
    if predictor != 1:
        _refuse(path, f"the JPEG scan selects predictor {predictor} (Ss): only predictor 1 (first-order, from the left neighbour) is read; "
                      "predictors 2-7 are out of scope")
    if transform & 15:
        _refuse(path, f"the JPEG scan sets a point transform of {transform & 15} (Al): only 0 is read")
    if not 2 <= precision <= 16:
        _refuse(path, f"malformed: JPEG precision {precision} (P) outside 2..16")
    if precision > f.bits_allocated or precision < f.bits_stored:
        _refuse(path, f"JPEG precision {precision} (P) outside BitsStored {f.bits_stored} .. BitsAllocated {f.bits_allocated}")
    if (lines, samples) != (f.rows, f.columns):
        _refuse(path, f"the JPEG frame is {lines} lines of {samples} samples, Rows and Columns say {f.rows} x {f.columns}")
    if table >> 4 not in tables:
        _refuse(path, f"malformed: the JPEG scan selects Huffman table {table >> 4}, for which the stream holds no DHT (it defines {sorted(tables)})")
    bits, values = tables[table >> 4]
    f.jpeg = JpegScan(int(precision), int(lines), int(samples), bits, values, behind - at, end - behind)
    return at, length


def read_file(path, header_only=False) -> DicomFile:
    """Parse one file up to PixelData (7FE0,0010).  `frame` is a zero-copy uint8 view of the file's voxel bytes, or of its RLE or JPEG
    fragment (the file stays mapped while the view lives); with `header_only` everything is parsed and checked alike, no voxel byte is read and
    `frame` stays None."""
    with part10(path) as p:
        path, buf, size, off = p.path, p.buf, p.size, p.off
        explicit, encoding = _check_syntax(p.syntax, path, jpeg_lossless=True)
        f = DicomFile(path, p.syntax, encoding=encoding)
        while off < size:
            tag, vr, length, voff = _element(buf, off, explicit, path)
            if tag in (FLOAT_PIXEL_DATA, DOUBLE_PIXEL_DATA):
                _refuse(path, f"{'float' if tag == FLOAT_PIXEL_DATA else 'double float'} pixel data ({tag[0]:04X},{tag[1]:04X}) is outside the path: "
                              "only integer PixelData (7FE0,0010) is read")
            if tag == PIXEL_DATA:
                f.pixel_offset, f.pixel_length = voff, length
                break
            if tag > PIXEL_DATA:
                break
            if tag[0] == 0xFFFE:
                _refuse(path, f"malformed: item tag ({tag[0]:04X},{tag[1]:04X}) at byte {off} outside a sequence")
            if length == UNDEFINED:
                off = _skip_sequence(buf, voff, explicit and vr != "UN", path)
                continue
            if voff + length > size:
                _refuse(path, f"malformed: element ({tag[0]:04X},{tag[1]:04X}) at byte {off} declares {length} bytes, {size - voff} are left")
            if tag in KEPT:
                name, kvr = KEPT[tag]
                v = _value(buf, name, kvr, voff, length, path)
                if v is not None:
                    setattr(f, name, v)
            off = voff + length
        if f.has_image:
            need, at = _validate(f, size), f.pixel_offset
            if encoding == RLE:
                at, need = _rle_fragment(buf, f, size)
            if encoding == JPEGLL:
                at, need = _jpeg_fragment(buf, f, size)
            if not header_only:
                f.frame = np.frombuffer(buf, dtype=np.uint8, count=need, offset=at)
                p.keep = True
    return f


@dataclass
class DicomSeries:
    """A sorted series: what `ingest.decode_series` uploads.  `shape`: (Columns, Rows, slices) = the extents along voxel index (i, j, k);
    `affine`: 4x4 float64 voxel index -> mm in RAS, or None (a single slice without geometry); `slopes`, `inters`: RescaleSlope /
    RescaleIntercept per sorted slice; `frames`: per sorted slice a uint8 view of that file's PixelData bytes (empty with header_only);
    `encoding`: NATIVE, or RLE: `frames` are the files' RLE fragments and `segments` holds per sorted slice the (bits_allocated / 8, 2)
    int64 table of each segment's byte offset into its fragment and byte length, or JPEGLL: `frames` are the files' JPEG fragments and
    `jpeg` holds per sorted slice its `JpegScan`."""
    shape: Tuple[int, int, int]
    affine: Optional[np.ndarray]
    path: str
    bits_allocated: int
    bits_stored: int
    high_bit: int
    signed: bool
    slopes: List[float]
    inters: List[float]
    frames: List[np.ndarray] = field(default_factory=list)
    files: List[str] = field(default_factory=list)       # the slices' paths in sorted order
    encoding: str = NATIVE
    segments: List[np.ndarray] = field(default_factory=list)
    jpeg: List[JpegScan] = field(default_factory=list)

    def uniform_scale(self):
        """(slope, inter) when every slice carries the same pair bit for bit, else None."""
        pairs = {(struct.pack("<d", s), struct.pack("<d", i)) for s, i in zip(self.slopes, self.inters)}
        return (float(self.slopes[0]), float(self.inters[0])) if len(pairs) == 1 else None


def series_directory(directory):
    """`directory` itself when it holds regular files, else its single sub-directory (upstream takes `os.listdir(...)[0]`)."""
    directory = str(directory)
    if not os.path.isdir(directory):
        raise ConfigurationError(f"{directory}: not a directory, so no DICOM series can be read from it")
    entries = sorted(e for e in os.listdir(directory) if not e.startswith("."))
    if any(os.path.isfile(os.path.join(directory, e)) for e in entries):
        return directory
    dirs = [e for e in entries if os.path.isdir(os.path.join(directory, e))]
    if len(dirs) > 1:
        raise ConfigurationError(f"{directory}: {len(dirs)} sub-directories ({', '.join(dirs[:4])}{', ...' if len(dirs) > 4 else ''}) and no files: "
                                 "one series directory is expected")
    if not dirs:
        raise ConfigurationError(f"{directory}: no DICOM files")
    inner = os.path.join(directory, dirs[0])
    if not any(os.path.isfile(os.path.join(inner, e)) for e in os.listdir(inner) if not e.startswith(".")):
        raise ConfigurationError(f"{inner}: no DICOM files")
    return inner


def _geometry(slices, directory):
    """(slices sorted along the normal, LPS 4x4 matrix or None)."""
    z = len(slices)
    missing = [(s, n) for s in slices for n in ("position", "orientation", "pixel_spacing") if getattr(s, n) is None]
    if missing:
        if z > 1:
            s, n = missing[0]
            names = {"position": "ImagePositionPatient", "orientation": "ImageOrientationPatient", "pixel_spacing": "PixelSpacing"}
            _refuse(s.path, f"no {names[n]} in a series of {z} slices: without geometry neither the slice order nor a resampling map exists")
        return slices, None
    first = slices[0]
    ori = np.asarray(first.orientation, dtype=np.float64)
    for s in slices[1:]:
        if np.abs(np.asarray(s.orientation, dtype=np.float64) - ori).max() > 1e-4:
            raise ConfigurationError(f"{directory}: {first.path} and {s.path} differ in ImageOrientationPatient ({first.orientation} and {s.orientation})")
    r, c = ori[:3], ori[3:]
    n = np.cross(r, c)
    if not np.isfinite(ori).all() or np.linalg.norm(n) < 1e-6:
        _refuse(first.path, f"ImageOrientationPatient {first.orientation} spans no plane")
    along = [float(n @ np.asarray(s.position, dtype=np.float64)) for s in slices]
    order = sorted(range(z), key=lambda i: along[i])
    slices = [slices[i] for i in order]
    along = [along[i] for i in order]
    gaps = np.diff(along)
    for i, g in enumerate(gaps):
        if g < 1e-6:
            raise ConfigurationError(f"{directory}: duplicate position: {slices[i].path} and {slices[i + 1].path} lie {g:.3g} mm apart along the slice normal")
    if z > 2 and np.abs(gaps - gaps.mean()).max() > 0.01 * gaps.mean():
        logger.warning("%s: non-uniform slice spacing (gaps between %.6g and %.6g mm, mean %.6g): the volume is read as if the slices were "
                       "evenly spaced between the first and the last", directory, gaps.min(), gaps.max(), gaps.mean())
    first, last = slices[0], slices[-1]
    p0 = np.asarray(first.position, dtype=np.float64)
    m = np.eye(4, dtype=np.float64)
    m[:3, 0] = r * first.pixel_spacing[1]
    m[:3, 1] = c * first.pixel_spacing[0]
    if z > 1:
        m[:3, 2] = (np.asarray(last.position, dtype=np.float64) - p0) / (z - 1)
    else:
        step = first.spacing_between_slices or first.slice_thickness or 1.0
        m[:3, 2] = n * step
    m[:3, 3] = p0
    return slices, m


def read_series(directory, header_only=False) -> DicomSeries:
    """The series under `directory` (see `series_directory`), sorted by position.  Files without the magic or without Rows / PixelData
    (a DICOMDIR, a report) are skipped; of several SeriesInstanceUIDs the first in sorted order is read."""
    d = series_directory(directory)
    slices, skipped = [], 0
    for name in sorted(os.listdir(d)):
        p = os.path.join(d, name)
        if name.startswith(".") or not os.path.isfile(p):
            continue
        try:
            f = read_file(p, header_only)
        except NotDicomError:
            skipped += 1
            continue
        if not f.has_image:
            skipped += 1
            continue
        slices.append(f)
    if skipped:
        logger.info("%s: %d file(s) without the DICM magic or without an image skipped", d, skipped)
    if not slices:
        raise ConfigurationError(f"{d}: no DICOM image files ({skipped} file(s) without the DICM magic or without Rows / PixelData skipped)")
    uids = sorted({s.series_uid or "" for s in slices})
    if len(uids) > 1:
        logger.warning("%s: %d SeriesInstanceUIDs; %s is read, ignored: %s", d, len(uids), uids[0], ", ".join(uids[1:]))
        slices = [s for s in slices if (s.series_uid or "") == uids[0]]
    first = slices[0]
    for s in slices[1:]:
        for name, what in (("rows", "Rows"), ("columns", "Columns"), ("bits_allocated", "BitsAllocated"), ("bits_stored", "BitsStored"),
                           ("high_bit", "HighBit"), ("pixel_representation", "PixelRepresentation")):
            if getattr(s, name) != getattr(first, name):
                raise ConfigurationError(f"{d}: {first.path} and {s.path} differ in {what} ({getattr(first, name)} and {getattr(s, name)})")
        if s.encoding != first.encoding:
            raise ConfigurationError(f"{d}: {first.path} ({first.transfer_syntax}) and {s.path} ({s.transfer_syntax}) mix uncompressed, RLE "
                                     "lossless and JPEG lossless files in one series")
    slices, lps = _geometry(slices, d)
    affine = None if lps is None else lps_to_ras(lps)
    first = slices[0]
    return DicomSeries((int(first.columns), int(first.rows), len(slices)), affine, d, int(first.bits_allocated), int(first.bits_stored),
                       int(first.high_bit), bool(first.pixel_representation), [float(s.slope) for s in slices], [float(s.inter) for s in slices],
                       [] if header_only else [s.frame for s in slices], [s.path for s in slices], first.encoding,
                       [s.segments for s in slices] if first.encoding == RLE else [],
                       [s.jpeg for s in slices] if first.encoding == JPEGLL else [])
