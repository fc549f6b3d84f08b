"""A minimal DICOM writer and the DICOM twin of a `synth_nifti.write_tree` tree, for the tests, the timing tool and a first run of
`main.py --image_loc` on the DICOM layout (`mmnn_sts_amd.data.ImageDatasets`).  A test and demo aid, like `synth_nifti`: it writes what
`mmnn_sts_amd.data.dicom` reads (one frame per file; uncompressed in explicit VR little endian, or implicit on request, RLE Lossless
with `transfer_syntax="rle"`, or JPEG Lossless with first-order prediction, 1.2.840.10008.1.2.4.70, with `transfer_syntax="jpeg-lossless"`)
and nothing else.

    <root>/images/t1/SYN-0007-t1-a/image/series_1/0003.dcm ...     one file per slice, names in a seeded random order
    <root>/images/t1/SYN-0007-t1-a/mask/series_1/0011.dcm ...      the mask as an 8-bit image series, 0 / 255
    <root>/images/t1/SYN-0007-t1-a/mask/rtstruct.dcm               with mask_format="rtstruct": the mask as one RT Structure Set file
    <root>/images/t1/SYN-0007-t1-a/mask/seg.dcm                    with mask_format="seg": the mask as one BINARY Segmentation object
    <root>/key.csv, clinical.csv, train_uids.txt, val_uids.txt     copied from the NIfTI tree

    python -m mmnn_sts_amd.data.synth_dicom NIFTI_DIR DICOM_DIR [--mask_format rtstruct | seg] [--transfer_syntax rle | jpeg-lossless]

The twin holds the same voxels -- slice k, row j, column i is the NIfTI voxel (i, j, k) -- and the same geometry: ImagePositionPatient,
ImageOrientationPatient and PixelSpacing are the NIfTI affine's columns in LPS (a sheared or left-handed affine has no such form and is
refused).  Decimal strings hold at most 16 characters, as the standard says, so the geometry agrees with the NIfTI header's to about
1e-10 relative, not bit for bit.
"""
import argparse
import os
import shutil
import struct

import numpy as np

from ..exceptions.exceptions import ConfigurationError
from . import nifti
from .dicom import EXPLICIT_LE, IMPLICIT_LE, JPEG_LOSSLESS_SV1, LONG_VRS, RLE_LOSSLESS

MR_IMAGE_STORAGE = "1.2.840.10008.5.1.4.1.1.4"
RT_STRUCTURE_SET_STORAGE = "1.2.840.10008.5.1.4.1.1.481.3"
SEGMENTATION_STORAGE = "1.2.840.10008.5.1.4.1.1.66.4"
MASK_FORMATS = ("series", "rtstruct", "seg")
TRANSFER_SYNTAXES = ("native", "rle", "jpeg-lossless")
# T.81 Table K.3 (luminance DC) extended by one code per length up to 14 bits, so that it covers the categories 0..16: Kraft sum 1 - 2^-14
JPEG_DEFAULT_TABLE = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0), tuple(range(17)))
JPEG_TABLES = ("default", "frame")
UID_ROOT = "1.2.3.4.5"                       # not a registered root: synthetic files only


def ds(value) -> str:
    """A decimal string of at most 16 characters: the shortest repr when it fits, else the most significant digits that do."""
    value = float(value)
    text = repr(value)
    if text.endswith(".0"):
        text = text[:-2]
    digits = 17
    while len(text) > 16 and digits > 1:
        digits -= 1
        text = f"{value:.{digits}g}"
    return text


def _element(group, elem, vr, value: bytes, explicit: bool) -> bytes:
    if len(value) % 2:
        value += b"\0" if vr in ("UI", "OB", "OW", "UN") else b" "
    if not explicit:
        return struct.pack("<HHI", group, elem, len(value)) + value
    if vr in LONG_VRS:
        return struct.pack("<HH2sHI", group, elem, vr.encode(), 0, len(value)) + value
    return struct.pack("<HH2sH", group, elem, vr.encode(), len(value)) + value


def _text(values) -> bytes:
    return "\\".join(values if isinstance(values, (list, tuple)) else [values]).encode("ascii")


def packbits(row) -> bytes:
    """One row of bytes as PackBits runs (PS3.5 G.3.1): a stretch of 2 or more equal bytes becomes repeat runs (control byte 257 - n,
    n <= 128, then the byte; a single byte left over becomes a literal of one), the bytes between such stretches literal runs (control
    byte n - 1, n <= 128, then the n bytes)."""
    row = np.ascontiguousarray(row, dtype=np.uint8).reshape(-1)
    n = row.size
    if n == 0:
        return b""
    starts = np.concatenate(([0], np.flatnonzero(row[1:] != row[:-1]) + 1))
    lengths = np.diff(np.concatenate((starts, [n])))
    repeats = np.flatnonzero(lengths >= 2)
    out = bytearray()
    k, m = 0, len(starts)
    while k < m:
        if lengths[k] >= 2:
            value, left = int(row[starts[k]]), int(lengths[k])
            while left >= 2:
                take = min(left, 128)
                out += bytes((257 - take, value))
                left -= take
            if left:
                out += bytes((0, value))
            k += 1
            continue
        j = np.searchsorted(repeats, k)                                                  # the next stretch of equal bytes
        j = int(repeats[j]) if j < len(repeats) else m
        a, b = int(starts[k]), (int(starts[j]) if j < m else n)
        for at in range(a, b, 128):
            piece = row[at:min(at + 128, b)]
            out += bytes((piece.size - 1,)) + piece.tobytes()
        k = j
    return bytes(out)


def rle_fragment(pixels) -> bytes:
    """A (Rows, Columns) frame as one RLE fragment (PS3.5 Annex G): the 64-byte header (the segment count and 15 offsets from the start
    of the header, unused ones zero), then one segment per byte of the word, the most significant byte plane first, every row encoded
    on its own (`packbits`) and every segment padded with a zero byte to even length."""
    a = np.ascontiguousarray(pixels)
    planes = a.astype(a.dtype.newbyteorder("<")).view(np.uint8).reshape(a.shape[0], a.shape[1], a.dtype.itemsize)
    segments = []
    for s in range(a.dtype.itemsize):
        data = b"".join(packbits(row) for row in planes[:, :, a.dtype.itemsize - 1 - s])
        segments.append(data + b"\0" * (len(data) % 2))
    offsets, at = [], 64
    for seg in segments:
        offsets.append(at)
        at += len(seg)
    return struct.pack("<16I", len(segments), *offsets, *([0] * (15 - len(offsets)))) + b"".join(segments)


def jpeg_categories(pixels, precision):
    """(SSSS, extra bits) per sample of a (Rows, Columns) frame under predictor 1 (T.81 H.1.2): the first sample is predicted 2^(P-1),
    the rest of the first row from the left, the first sample of a later row from above, every other sample from the left.  The
    difference is taken modulo 2^16 into -32767..32768; its category SSSS is 0 for 0, 16 for 32768, else the bit length of its
    magnitude, and its SSSS extra bits are the difference, or the difference + 2^SSSS - 1 when it is negative (none for 0 and 16)."""
    a = np.ascontiguousarray(pixels)
    words = a.view(np.dtype(f"u{a.dtype.itemsize}")).astype(np.int64)
    predicted = np.empty_like(words)
    predicted[:, 1:] = words[:, :-1]
    predicted[1:, 0] = words[:-1, 0]
    predicted[0, 0] = 1 << (precision - 1)
    d = ((words - predicted) & 0xFFFF).reshape(-1)
    d = np.where(d > 32768, d - 65536, d)
    magnitude = np.abs(d)
    ssss = np.zeros(d.shape, dtype=np.int64)
    for s in range(1, 17):
        ssss[magnitude >= 1 << (s - 1)] = s
    extra = np.where(d >= 0, d, d + (1 << ssss) - 1)
    extra[ssss == 16] = 0
    return ssss, extra


def canonical_codes(bits, huffval):
    """{value: (code, length)} of a BITS / HUFFVAL pair as T.81 Annex C assigns them."""
    codes, code, k = {}, 0, 0
    for length, count in enumerate(bits, 1):
        for _ in range(int(count)):
            codes[int(huffval[k])] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def frame_table(ssss):
    """A Huffman table of a frame's own category counts, the code lengths limited to 16: the lengths of a Huffman tree over the
    categories that occur (a lone one gets a one-bit code), then, while a length exceeds 16 or the all-ones code is in use (T.81 forbids
    it: Kraft sum 1), the rarest symbols are pushed down and the sum restored by lengthening the shortest code that can pay for it."""
    counts = np.bincount(ssss, minlength=17)
    present = [int(v) for v in np.flatnonzero(counts)]
    lengths = {v: 0 for v in present}
    heap = sorted((int(counts[v]), [v]) for v in present)
    while len(heap) > 1:
        (ca, a), (cb, b) = heap[0], heap[1]
        for v in a + b:
            lengths[v] += 1
        heap = sorted(heap[2:] + [(ca + cb, a + b)])
    rare = min(present, key=lambda v: (counts[v], -v))
    lengths[rare] += 1                         # one code point left over: the all-ones code stays free
    order = sorted(present, key=lambda v: (lengths[v], -counts[v], v))
    for v in order:
        lengths[v] = min(lengths[v], 16)
    kraft = lambda: sum(1 << (16 - lengths[v]) for v in present)
    while kraft() > (1 << 16) - 1:             # the clamp over-subscribed the code: lengthen the longest code that is still below 16
        v = max((v for v in present if lengths[v] < 16), key=lambda v: (lengths[v], -counts[v]))
        lengths[v] += 1
    order = sorted(present, key=lambda v: (lengths[v], v))
    bits = [sum(1 for v in present if lengths[v] == l) for l in range(1, 17)]
    return tuple(bits), tuple(order)


def jpeg_entropy(ssss, extra, table) -> bytes:
    """The entropy-coded data of a scan: per sample the code of its category, then its extra bits, most significant bit first; the last
    byte padded with 1-bits; a zero byte stuffed behind every FF."""
    codes = canonical_codes(*table)
    code_of, length_of = np.zeros(17, dtype=np.int64), np.zeros(17, dtype=np.int64)
    for v, (code, length) in codes.items():
        code_of[v], length_of[v] = code, length
    if (length_of[ssss] == 0).any():
        raise ConfigurationError(f"the Huffman table has no code for category {int(ssss[length_of[ssss] == 0][0])}")
    more = np.where(ssss == 16, 0, ssss)
    word = (code_of[ssss] << more) | extra
    width = length_of[ssss] + more
    start = np.concatenate(([0], np.cumsum(width)))
    stream = np.ones((int(start[-1]) + 7) // 8 * 8, dtype=np.uint8)
    for j in range(int(width.max()) if width.size else 0):
        has = width > j
        stream[start[:-1][has] + j] = (word[has] >> (width[has] - 1 - j)) & 1
    data = np.packbits(stream)
    return np.insert(data, np.flatnonzero(data == 0xFF) + 1, 0).tobytes()


def jpeg_lossless_fragment(pixels, bits_stored=None, table="default") -> bytes:
    """A (Rows, Columns) frame of 8 or 16-bit words as one JPEG Lossless stream (T.81 Annex H, predictor 1): SOI, DHT, SOF3, SOS, the
    entropy-coded data (`jpeg_entropy`) and EOI.  The precision P is `bits_stored` when no word has a bit set above it, else the
    word's width.  `table`: 'default' (`JPEG_DEFAULT_TABLE`), 'frame' (`frame_table` of this frame) or a (BITS, HUFFVAL) pair."""
    a = np.ascontiguousarray(pixels)
    if a.dtype.itemsize not in (1, 2):
        raise ConfigurationError(f"JPEG Lossless holds samples of at most 16 bits, got {a.dtype}")
    width = a.dtype.itemsize * 8
    words = a.view(np.dtype(f"u{a.dtype.itemsize}"))
    precision = width if bits_stored is None or int(bits_stored) >= width or int(words.max()) >> int(bits_stored) else max(int(bits_stored), 2)
    ssss, extra = jpeg_categories(a, precision)
    if isinstance(table, str):
        if table not in JPEG_TABLES:
            raise ConfigurationError(f"jpeg_table {table!r} is none of {JPEG_TABLES}")
        table = JPEG_DEFAULT_TABLE if table == "default" else frame_table(ssss)
    bits, huffval = table
    dht = bytes([0x00]) + bytes(int(v) for v in bits) + bytes(int(v) for v in huffval)
    sof = struct.pack(">BHHB", precision, a.shape[0], a.shape[1], 1) + bytes([1, 0x11, 0])
    sos = bytes([1, 1, 0x00, 1, 0, 0])         # one component, table 0; Ss = 1: the predictor; Se = 0; Ah, Al = 0
    segment = lambda marker, body: bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body
    data = b"\xff\xd8" + segment(0xC4, dht) + segment(0xC3, sof) + segment(0xDA, sos) + jpeg_entropy(ssss, extra, table) + b"\xff\xd9"
    return data + b"\0" * (len(data) % 2)


def _encapsulated(fragment: bytes) -> bytes:
    """PixelData of undefined length (explicit VR): an empty Basic Offset Table, one fragment, the sequence delimiter."""
    return (struct.pack("<HH2sHI", 0x7FE0, 0x0010, b"OB", 0, 0xFFFFFFFF) + struct.pack("<HHI", 0xFFFE, 0xE000, 0)
            + struct.pack("<HHI", 0xFFFE, 0xE000, len(fragment)) + fragment + struct.pack("<HHI", 0xFFFE, 0xE0DD, 0))


def file_bytes(pixels, bits_stored=None, high_bit=None, position=None, orientation=None, pixel_spacing=None, slope=None, inter=None,
               series_uid=UID_ROOT + ".1", instance_number=1, explicit=True, slice_thickness=None, spacing_between_slices=None,
               sop_instance_uid=UID_ROOT + ".1.1", transfer_syntax="native", jpeg_table="default") -> bytes:
    """One slice as a part-10 file.  `pixels`: a (Rows, Columns) array of uint8 / int8 / uint16 / int16 / uint32 / int32, written as
    it is (the caller has placed the stored bits); geometry and rescale elements are left out when None.  `transfer_syntax` 'rle':
    RLE Lossless, whose data set is explicit VR and whose PixelData is encapsulated (`rle_fragment`); 'jpeg-lossless': JPEG Lossless
    with first-order prediction, encapsulated alike (`jpeg_lossless_fragment` with `jpeg_table`), of 8 or 16-bit words."""
    a = np.ascontiguousarray(pixels)
    if a.ndim != 2 or a.dtype.kind not in "iu" or a.dtype.itemsize not in (1, 2, 4):
        raise ConfigurationError(f"a slice is a 2-D array of 8, 16 or 32-bit integers, got {a.dtype} {a.shape}")
    if transfer_syntax not in TRANSFER_SYNTAXES:
        raise ConfigurationError(f"transfer_syntax {transfer_syntax!r} is none of {TRANSFER_SYNTAXES}")
    if transfer_syntax != "native" and not explicit:
        raise ConfigurationError(f"an {'RLE' if transfer_syntax == 'rle' else 'JPEG'} Lossless data set is explicit VR little endian: explicit=False "
                                 "cannot be combined with it")
    bits = a.dtype.itemsize * 8
    bits_stored = bits if bits_stored is None else int(bits_stored)
    high_bit = bits_stored - 1 if high_bit is None else int(high_bit)
    us = lambda v: struct.pack("<H", v)
    syntax = {"rle": RLE_LOSSLESS, "jpeg-lossless": JPEG_LOSSLESS_SV1}.get(transfer_syntax, EXPLICIT_LE if explicit else IMPLICIT_LE)
    meta = b"".join([_element(0x0002, 0x0001, "OB", b"\0\1", True), _element(0x0002, 0x0002, "UI", _text(MR_IMAGE_STORAGE), True),
                     _element(0x0002, 0x0003, "UI", _text(sop_instance_uid), True), _element(0x0002, 0x0010, "UI", _text(syntax), True),
                     _element(0x0002, 0x0012, "UI", _text(UID_ROOT + ".0"), True)])
    meta = _element(0x0002, 0x0000, "UL", struct.pack("<I", len(meta)), True) + meta
    e = []
    add = lambda g, el, vr, v: e.append(_element(g, el, vr, v, explicit))
    add(0x0008, 0x0016, "UI", _text(MR_IMAGE_STORAGE))
    add(0x0008, 0x0018, "UI", _text(sop_instance_uid))
    add(0x0008, 0x0060, "CS", b"MR")
    if slice_thickness is not None:
        add(0x0018, 0x0050, "DS", _text(ds(slice_thickness)))
    if spacing_between_slices is not None:
        add(0x0018, 0x0088, "DS", _text(ds(spacing_between_slices)))
    add(0x0020, 0x000E, "UI", _text(series_uid))
    add(0x0020, 0x0013, "IS", _text(str(int(instance_number))))
    if position is not None:
        add(0x0020, 0x0032, "DS", _text([ds(v) for v in position]))
    if orientation is not None:
        add(0x0020, 0x0037, "DS", _text([ds(v) for v in orientation]))
    add(0x0028, 0x0002, "US", us(1))
    add(0x0028, 0x0004, "CS", b"MONOCHROME2")
    add(0x0028, 0x0010, "US", us(a.shape[0]))
    add(0x0028, 0x0011, "US", us(a.shape[1]))
    if pixel_spacing is not None:
        add(0x0028, 0x0030, "DS", _text([ds(v) for v in pixel_spacing]))
    add(0x0028, 0x0100, "US", us(bits))
    add(0x0028, 0x0101, "US", us(bits_stored))
    add(0x0028, 0x0102, "US", us(high_bit))
    add(0x0028, 0x0103, "US", us(1 if a.dtype.kind == "i" else 0))
    if inter is not None:
        add(0x0028, 0x1052, "DS", _text(ds(inter)))
    if slope is not None:
        add(0x0028, 0x1053, "DS", _text(ds(slope)))
    if transfer_syntax == "rle":
        e.append(_encapsulated(rle_fragment(a)))
    elif transfer_syntax == "jpeg-lossless":
        e.append(_encapsulated(jpeg_lossless_fragment(a, bits_stored, jpeg_table)))
    else:
        add(0x7FE0, 0x0010, "OB" if bits == 8 else "OW", a.astype(a.dtype.newbyteorder("<")).tobytes())
    return b"\0" * 128 + b"DICM" + meta + b"".join(e)


def lps_geometry(affine, what=""):
    """(orientation (6), pixel_spacing (2), first position (3), slice step (3)) of a RAS voxel-index -> mm matrix whose axes are
    (column, row, slice).  Refused: axes that are not orthogonal (shear) or not right-handed along the slice normal."""
    a = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    lps = np.diag([-1.0, -1.0, 1.0, 1.0]) @ a
    c0, c1, c2, t = lps[:3, 0], lps[:3, 1], lps[:3, 2], lps[:3, 3]
    s0, s1, s2 = (float(np.linalg.norm(v)) for v in (c0, c1, c2))
    if min(s0, s1, s2) <= 0.0:
        raise ConfigurationError(f"{what}: the affine has a zero column")
    r, c = c0 / s0, c1 / s1
    n = np.cross(r, c)
    if abs(float(r @ c)) > 1e-6 or np.linalg.norm(c2 - (n @ c2) * n) > 1e-6 * s2 or float(n @ c2) <= 0.0:
        raise ConfigurationError(f"{what}: a sheared or left-handed affine has no ImageOrientationPatient / ImagePositionPatient form")
    return tuple(r) + tuple(c), (s1, s0), t, c2


def _stored(volume, bits_stored, rng):
    """`volume` with its values in the low `bits_stored` bits and seeded garbage in the unused high bits of every word."""
    bits = volume.dtype.itemsize * 8
    if bits_stored is None or bits_stored == bits:
        return volume
    lo, hi = (-(1 << (bits_stored - 1)), (1 << (bits_stored - 1)) - 1) if volume.dtype.kind == "i" else (0, (1 << bits_stored) - 1)
    if volume.min() < lo or volume.max() > hi:
        raise ConfigurationError(f"the voxels span {volume.min()}..{volume.max()}: they do not fit {bits_stored} stored bits")
    unsigned = np.dtype(f"u{volume.dtype.itemsize}")
    word = volume.view(unsigned) & unsigned.type((1 << bits_stored) - 1)
    garbage = rng.integers(0, 1 << (bits - bits_stored), volume.shape, dtype=np.uint64).astype(unsigned) << unsigned.type(bits_stored)
    return (word | garbage).view(volume.dtype)


def write_series(directory, volume, affine=None, slope=None, inter=None, series_uid=UID_ROOT + ".1", shuffle_names=True, seed=0,
                 bits_stored=None, per_slice_scale=False, explicit=True, transfer_syntax="native", jpeg_table="default"):
    """Write the (x, y, z) integer `volume` as z slice files under `directory`.  `per_slice_scale`: slice k carries its own pair,
    slope (1 + (k % 4) / 8) and inter - 3.5 k, so that the series has no shared scale.  `transfer_syntax`: 'native' (uncompressed),
    'rle' (RLE Lossless) or 'jpeg-lossless' (with `jpeg_table`, see `jpeg_lossless_fragment`)."""
    volume = np.asarray(volume)
    if volume.ndim != 3:
        raise ConfigurationError(f"a volume has three axes, got {volume.shape}")
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng([int(seed), 7])
    orientation, spacing, first, step = lps_geometry(affine, directory)
    z = volume.shape[2]
    names = rng.permutation(z) if shuffle_names else np.arange(z)
    numbers = rng.permutation(z) if shuffle_names else np.arange(z)
    words = _stored(volume, bits_stored, rng)
    for k in range(z):
        s, i = slope, inter
        if per_slice_scale:
            s, i = (1.0 if slope is None else slope) * (1.0 + (k % 4) / 8.0), (0.0 if inter is None else inter) - 3.5 * k
        data = file_bytes(words[:, :, k].T, bits_stored, None, first + k * step, orientation, spacing, s, i, series_uid, int(numbers[k]) + 1,
                          explicit, float(np.linalg.norm(step)), float(np.linalg.norm(step)), f"{series_uid}.{k + 1}", transfer_syntax, jpeg_table)
        with open(os.path.join(directory, f"{int(names[k]):04d}.dcm"), "wb") as f:
            f.write(data)
    return directory


def _sequence(group, elem, items, explicit, undefined):
    """A sequence element: `items` are the encoded data sets of its items; `undefined`: sequence and items of undefined length, closed
    by their delimiters."""
    if undefined:
        body = b"".join(struct.pack("<HHI", 0xFFFE, 0xE000, 0xFFFFFFFF) + it + struct.pack("<HHI", 0xFFFE, 0xE00D, 0) for it in items)
        body += struct.pack("<HHI", 0xFFFE, 0xE0DD, 0)
        head = struct.pack("<HH2sHI", group, elem, b"SQ", 0, 0xFFFFFFFF) if explicit else struct.pack("<HHI", group, elem, 0xFFFFFFFF)
        return head + body
    return _element(group, elem, "SQ", b"".join(struct.pack("<HHI", 0xFFFE, 0xE000, len(it)) + it for it in items), explicit)


def rtstruct_bytes(rois, explicit=True, undefined_lengths=False, frame_uid=UID_ROOT + ".9", sop_instance_uid=UID_ROOT + ".8.1") -> bytes:
    """An RT Structure Set as a part-10 file.  `rois`: [(name, [(geometric type, (n, 3) points in LPS mm), ...]), ...]; a contour may
    carry a third entry, the NumberOfContourPoints to declare in place of n.  Coordinates are written with `ds()`.  A ContourData
    value too long for the 16-bit length of an explicit-VR DS element is written as UN with a 32-bit length (PS3.5 6.2.2)."""
    def el(g, e, vr, v):
        if explicit and vr not in LONG_VRS and len(v) > 0xFFFE:
            vr = "UN"
        return _element(g, e, vr, v, explicit)

    syntax = EXPLICIT_LE if explicit else IMPLICIT_LE
    meta = b"".join([_element(0x0002, 0x0001, "OB", b"\0\1", True), _element(0x0002, 0x0002, "UI", _text(RT_STRUCTURE_SET_STORAGE), True),
                     _element(0x0002, 0x0003, "UI", _text(sop_instance_uid), True), _element(0x0002, 0x0010, "UI", _text(syntax), True),
                     _element(0x0002, 0x0012, "UI", _text(UID_ROOT + ".0"), True)])
    meta = _element(0x0002, 0x0000, "UL", struct.pack("<I", len(meta)), True) + meta
    described, drawn = [], []
    for number, (name, contours) in enumerate(rois, 1):
        described.append(el(0x3006, 0x0022, "IS", _text(str(number))) + el(0x3006, 0x0024, "UI", _text(frame_uid)) + el(0x3006, 0x0026, "LO", _text(name)))
        items = []
        for kind, points, *declared in contours:
            points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
            count = declared[0] if declared else len(points)
            items.append(el(0x3006, 0x0042, "CS", _text(kind)) + el(0x3006, 0x0046, "IS", _text(str(int(count))))
                         + el(0x3006, 0x0050, "DS", _text([ds(v) for v in points.reshape(-1)])))
        drawn.append(el(0x3006, 0x002A, "IS", _text(["255", "0", "0"])) + _sequence(0x3006, 0x0040, items, explicit, undefined_lengths)
                     + el(0x3006, 0x0084, "IS", _text(str(number))))
    e = [el(0x0008, 0x0016, "UI", _text(RT_STRUCTURE_SET_STORAGE)), el(0x0008, 0x0018, "UI", _text(sop_instance_uid)), el(0x0008, 0x0060, "CS", b"RTSTRUCT"),
         el(0x3006, 0x0002, "SH", b"SYNTHETIC"), _sequence(0x3006, 0x0020, described, explicit, undefined_lengths),
         _sequence(0x3006, 0x0039, drawn, explicit, undefined_lengths)]
    return b"\0" * 128 + b"DICM" + meta + b"".join(e)


def run_rectangles(mask, affine):
    """A binary (x, y, z) mask as closed planar contours in LPS mm: one rectangle per run of set voxels in each row, with its corners
    at (i0 - 1/2, j - 1/2) ... (i1 + 1/2, j + 1/2) in voxel index coordinates, mapped through the RAS `affine`.  (A test device: a
    contouring workstation draws one polygon around a region, not one per run.)"""
    mask = np.asarray(mask) != 0
    if mask.ndim != 3:
        raise ConfigurationError(f"a mask has three axes, got {mask.shape}")
    a = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    edge = np.diff(np.pad(mask, ((1, 1), (0, 0), (0, 0))).astype(np.int8), axis=0)       # (x + 1, y, z): +1 where a run starts, -1 behind its end
    i0, j0, k0 = np.nonzero(edge == 1)
    order = np.lexsort((i0, j0, k0))
    i0, j0, k0 = i0[order], j0[order], k0[order]
    i1, j1, k1 = np.nonzero(edge == -1)
    order = np.lexsort((i1, j1, k1))
    i1 = i1[order]                                                                       # (the runs of a row pair up in order)
    lo, hi, top, bottom, k = i0 - 0.5, i1 - 0.5, j0 - 0.5, j0 + 0.5, k0.astype(np.float64)
    corners = np.stack([np.stack([lo, top, k], 1), np.stack([hi, top, k], 1), np.stack([hi, bottom, k], 1), np.stack([lo, bottom, k], 1)], 1)   # (runs, 4, 3)
    ras = corners @ a[:3, :3].T + a[:3, 3]
    lps = ras * np.array([-1.0, -1.0, 1.0])
    return [("CLOSED_PLANAR", p) for p in lps]


def write_rtstruct(path, mask, affine, roi_name="GTV", extra_rois=(), explicit=True, undefined_lengths=False):
    """Write the binary (x, y, z) `mask` as an RT Structure Set whose ROI `roi_name` holds one rectangle contour per run of set voxels
    (`run_rectangles`).  `extra_rois`: further ROIs written in front of and behind it alternately -- a name (a decoy: one rectangle
    around the whole first slice) or a (name, mask) pair."""
    rois = [(roi_name, run_rectangles(mask, affine))]
    for n, extra in enumerate(extra_rois):
        if isinstance(extra, str):
            decoy = np.zeros(np.asarray(mask).shape, dtype=np.uint8)
            decoy[:, :, 0] = 1
            extra = (extra, decoy)
        roi = (extra[0], run_rectangles(extra[1], affine))
        rois = [roi] + rois if n % 2 == 0 else rois + [roi]
    os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
    with open(path, "wb") as f:
        f.write(rtstruct_bytes(rois, explicit, undefined_lengths))
    return str(path)


def seg_bytes(rows, columns, segments, frames, pixel_data, orientation=None, pixel_spacing=None, step=None, explicit=True,
              undefined_lengths=False, per_frame_orientation=False, segmentation_type="BINARY", bits_allocated=1,
              sop_class=SEGMENTATION_STORAGE, number_of_frames=None, sop_instance_uid=UID_ROOT + ".7.1") -> bytes:
    """A Segmentation object as a part-10 file.  `segments`: [(SegmentNumber, SegmentLabel), ...]; `frames`: [(ReferencedSegmentNumber,
    ImagePositionPatient), ...] in the order of the frames in `pixel_data`, the PixelData value (bit-packed by the caller).
    `orientation` (6), `pixel_spacing` (2) and `step` (SliceThickness and SpacingBetweenSlices) go into the shared functional group,
    or, with `per_frame_orientation`, into every per-frame item; None leaves them out.  `number_of_frames`: the NumberOfFrames to
    declare in place of len(frames)."""
    el = lambda g, e, vr, v: _element(g, e, vr, v, explicit)
    seq = lambda g, e, items: _sequence(g, e, items, explicit, undefined_lengths)
    us = lambda v: struct.pack("<H", v)
    syntax = EXPLICIT_LE if explicit else IMPLICIT_LE
    meta = b"".join([_element(0x0002, 0x0001, "OB", b"\0\1", True), _element(0x0002, 0x0002, "UI", _text(sop_class), True),
                     _element(0x0002, 0x0003, "UI", _text(sop_instance_uid), True), _element(0x0002, 0x0010, "UI", _text(syntax), True),
                     _element(0x0002, 0x0012, "UI", _text(UID_ROOT + ".0"), True)])
    meta = _element(0x0002, 0x0000, "UL", struct.pack("<I", len(meta)), True) + meta
    measures = b""
    if step is not None:
        measures += el(0x0018, 0x0050, "DS", _text(ds(step))) + el(0x0018, 0x0088, "DS", _text(ds(step)))
    if pixel_spacing is not None:
        measures += el(0x0028, 0x0030, "DS", _text([ds(v) for v in pixel_spacing]))
    placed = b""                             # the functional groups that sit in the shared item or in every per-frame item, in tag order
    if orientation is not None:
        placed += seq(0x0020, 0x9116, [el(0x0020, 0x0037, "DS", _text([ds(v) for v in orientation]))])
    if measures:
        placed += seq(0x0028, 0x9110, [measures])
    per_frame = []
    for number, position in frames:
        item = seq(0x0020, 0x9113, [el(0x0020, 0x0032, "DS", _text([ds(v) for v in position]))])
        if per_frame_orientation:
            item += placed
        per_frame.append(item + seq(0x0062, 0x000A, [el(0x0062, 0x000B, "US", us(int(number)))]))
    described = [el(0x0062, 0x0004, "US", us(int(number))) + el(0x0062, 0x0005, "LO", _text(label)) + el(0x0062, 0x0008, "CS", b"MANUAL")
                 for number, label in segments]
    e = [el(0x0008, 0x0016, "UI", _text(sop_class)), el(0x0008, 0x0018, "UI", _text(sop_instance_uid)), el(0x0008, 0x0060, "CS", b"SEG"),
         el(0x0028, 0x0002, "US", us(1)), el(0x0028, 0x0004, "CS", b"MONOCHROME2"),
         el(0x0028, 0x0008, "IS", _text(str(len(frames) if number_of_frames is None else int(number_of_frames)))),
         el(0x0028, 0x0010, "US", us(rows)), el(0x0028, 0x0011, "US", us(columns)), el(0x0028, 0x0100, "US", us(bits_allocated)),
         el(0x0028, 0x0101, "US", us(bits_allocated)), el(0x0028, 0x0102, "US", us(bits_allocated - 1)), el(0x0028, 0x0103, "US", us(0)),
         el(0x0062, 0x0001, "CS", _text(segmentation_type)), seq(0x0062, 0x0002, described),
         seq(0x5200, 0x9229, [b"" if per_frame_orientation else placed]), seq(0x5200, 0x9230, per_frame),
         el(0x7FE0, 0x0010, "OB", bytes(pixel_data))]
    return b"\0" * 128 + b"DICM" + meta + b"".join(e)


def write_seg(path, mask, affine, label="GTV", extra_segments=(), explicit=True, undefined_lengths=False, shuffle_frames=True,
              per_frame_orientation=False, seed=0):
    """Write the binary (x, y, z) `mask`, on the grid of the RAS `affine`, as a BINARY Segmentation object whose segment `label` holds
    one frame per NON-EMPTY slice.  `extra_segments`: further segments -- a label (a decoy: the whole first slice) or a (label, mask)
    pair -- numbered in front of and behind it alternately, their frames interleaved with its own.  The frames are written in a
    seeded random order (`shuffle_frames`) and bit-packed back to back, least significant bit first, without byte alignment; the
    value is padded to even length, and the pad bits behind the last frame and the pad byte hold seeded garbage."""
    mask = np.asarray(mask) != 0
    if mask.ndim != 3:
        raise ConfigurationError(f"a mask has three axes, got {mask.shape}")
    x, y, z = mask.shape
    orientation, spacing, first, step = lps_geometry(affine, str(path))
    segments = [(label, mask)]
    for n, extra in enumerate(extra_segments):
        if isinstance(extra, str):
            decoy = np.zeros(mask.shape, dtype=bool)
            decoy[:, :, 0] = True
            extra = (extra, decoy)
        segment = (extra[0], np.asarray(extra[1]) != 0)
        segments = [segment] + segments if n % 2 == 0 else segments + [segment]
    frames = [(number, k) for number, (_, m) in enumerate(segments, 1) for k in range(z) if m[:, :, k].any()]
    rng = np.random.default_rng([int(seed), 11])
    if shuffle_frames:
        frames = [frames[i] for i in rng.permutation(len(frames))]
    bits = np.concatenate([segments[number - 1][1][:, :, k].T.reshape(-1) for number, k in frames]) if frames else np.zeros(0, dtype=bool)
    pad = -bits.size % 8
    packed = np.packbits(np.concatenate([bits, rng.integers(0, 2, pad).astype(bool)]), bitorder="little")
    if packed.size % 2:
        packed = np.concatenate([packed, rng.integers(0, 256, 1).astype(np.uint8)])
    data = seg_bytes(y, x, [(number, name) for number, (name, _) in enumerate(segments, 1)], [(number, first + k * step) for number, k in frames],
                     packed.tobytes(), orientation, spacing, float(np.linalg.norm(step)), explicit, undefined_lengths, per_frame_orientation)
    os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def from_nifti_tree(nifti_root, dicom_root, mask_value=255, shuffle_names=True, seed=0, bits_stored=None, per_slice_scale=False,
                    mask_format="series", roi_name="GTV", extra_rois=(), transfer_syntax="native", jpeg_table="default"):
    """The DICOM twin of a `synth_nifti.write_tree` tree; returns the same dictionary of locations.  Scans keep their type, slope and
    inter (as RescaleSlope / RescaleIntercept); non-zero mask voxels become `mask_value` (None: the mask's values are kept) in an 8-bit
    unsigned series.  `bits_stored`, `per_slice_scale`: of the scans (see `write_series`).  `mask_format` 'rtstruct': the mask directory
    holds one RT Structure Set file instead (`write_rtstruct` of the non-zero mask voxels on the scan's geometry, ROI `roi_name`,
    with `extra_rois`); the mask must then share the scan's extents.  `mask_format` 'seg': one BINARY Segmentation object
    instead (`write_seg` of the non-zero mask voxels, segment `roi_name`, with `extra_rois` as further segments), written on the
    mask's own grid when that is another than its scan's.  `transfer_syntax`, `jpeg_table`: of the scans and of the masks written as series."""
    if mask_format not in MASK_FORMATS:
        raise ConfigurationError(f"mask_format {mask_format!r} is none of {MASK_FORMATS}")
    nifti_root, dicom_root = str(nifti_root), str(dicom_root)
    src = os.path.join(nifti_root, "images")
    if not os.path.isdir(src):
        raise ConfigurationError(f"{nifti_root}: no images/ directory (a synth_nifti.write_tree tree is expected)")
    os.makedirs(dicom_root, exist_ok=True)
    out = {"image_loc": os.path.join(dicom_root, "images"), "t1_path": "t1", "t2_path": "t2"}
    for key, name in (("key_loc", "key.csv"), ("data_loc", "clinical.csv"), ("train_uids", "train_uids.txt"), ("val_uids", "val_uids.txt")):
        if os.path.exists(os.path.join(nifti_root, name)):
            shutil.copyfile(os.path.join(nifti_root, name), os.path.join(dicom_root, name))
            out[key] = os.path.join(dicom_root, name)
    count = 0
    for mod in sorted(os.listdir(src)):
        for patient in sorted(os.listdir(os.path.join(src, mod))):
            d = os.path.join(src, mod, patient)
            files = sorted(f for f in os.listdir(d) if not f.startswith("."))
            scans, masks = [f for f in files if f.startswith("scan")], [f for f in files if not f.startswith("scan")]
            if len(scans) != 1 or len(masks) != 1:
                raise ConfigurationError(f"{d}: one scan* file and one mask are expected")
            scan, mask = nifti.read(os.path.join(d, scans[0])), nifti.read(os.path.join(d, masks[0]))
            if scan.raw.dtype.kind not in "iu" or mask.raw.dtype.kind not in "iu":
                raise ConfigurationError(f"{d}: integer voxels are expected, got {scan.raw.dtype} and {mask.raw.dtype}")
            count += 1
            target = os.path.join(out["image_loc"], mod, patient)
            scaling = scan.scaling() or (None, None)
            write_series(os.path.join(target, "image", "series_1"), scan.raw, scan.affine, scaling[0], scaling[1], f"{UID_ROOT}.{count}.1",
                         shuffle_names, seed + 2 * count, bits_stored, per_slice_scale, transfer_syntax=transfer_syntax, jpeg_table=jpeg_table)
            if mask_format == "rtstruct":
                if mask.raw.shape != scan.raw.shape:
                    raise ConfigurationError(f"{d}: an RTSTRUCT twin is drawn on the scan's grid; the mask's extents {mask.raw.shape} differ from {scan.raw.shape}")
                write_rtstruct(os.path.join(target, "mask", "rtstruct.dcm"), mask.raw, scan.affine, roi_name, extra_rois)
                continue
            if mask_format == "seg":
                write_seg(os.path.join(target, "mask", "seg.dcm"), mask.raw, mask.affine, roi_name, extra_rois, shuffle_frames=shuffle_names,
                          seed=seed + 2 * count + 1)
                continue
            m = mask.raw if mask_value is None else np.where(mask.raw != 0, mask_value, 0)
            write_series(os.path.join(target, "mask", "series_1"), m.astype(np.uint8), mask.affine, None, None, f"{UID_ROOT}.{count}.2",
                         shuffle_names, seed + 2 * count + 1, transfer_syntax=transfer_syntax, jpeg_table=jpeg_table)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("nifti_dir", help="a synth_nifti.write_tree tree")
    ap.add_argument("dicom_dir")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bits_stored", type=int, default=None)
    ap.add_argument("--per_slice_scale", action="store_true")
    ap.add_argument("--mask_format", choices=MASK_FORMATS, default="series", help="the masks as 8-bit image series, as RT Structure Set files or as BINARY Segmentation objects")
    ap.add_argument("--transfer_syntax", choices=TRANSFER_SYNTAXES, default="native", help="of the scans and of the masks written as series: uncompressed, RLE Lossless, or JPEG Lossless with first-order prediction")
    ap.add_argument("--jpeg_table", choices=JPEG_TABLES, default="default", help="with --transfer_syntax jpeg-lossless: T.81 Table K.3 extended to 17 categories, "
                    "or a table from every frame's own category counts")
    a = ap.parse_args()
    for k, v in from_nifti_tree(a.nifti_dir, a.dicom_dir, seed=a.seed, bits_stored=a.bits_stored, per_slice_scale=a.per_slice_scale,
                                mask_format=a.mask_format, transfer_syntax=a.transfer_syntax, jpeg_table=a.jpeg_table).items():
        print(f"{k}: {v}")
