"""Helpers of the DICOM tests: the numpy restatement of the `mmnn_decode_slices` contract (include/mmnn_sts.h) and a struct-based packer
of part-10 files at the published element layout.  Shares no code with mmnn_sts_amd (neither the kernel's host side nor synth_dicom)."""
import struct

import numpy as np

IMPLICIT, EXPLICIT = "1.2.840.10008.1.2", "1.2.840.10008.1.2.1"
UNDEFINED = 0xFFFFFFFF
_LONG = ("OB", "OD", "OF", "OL", "OV", "OW", "SQ", "SV", "UC", "UN", "UR", "UT", "UV")
INTEGER_CODE = {(8, 0): 2, (8, 1): 256, (16, 0): 512, (16, 1): 4, (32, 0): 768, (32, 1): 8}
NP_OF_CODE = {2: "u1", 256: "i1", 512: "<u2", 4: "<i2", 768: "<u4", 8: "<i4", 64: "<f8"}


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def decode_ref(words, bits_stored, high_bit, signed, scale=None):
    """`words`: (x, y, z) unsigned array of the stored words.  u = (word >> (high_bit + 1 - bits_stored)) & (2^bits_stored - 1); v = u,
    or u sign-extended from bit bits_stored - 1; with `scale` ((z, 2) float64: slope, inter per slice) the float64 (v * slope) + inter,
    two roundings, else v in the integer type of the word's width and `signed`."""
    words = np.asarray(words)
    assert words.dtype.kind == "u" and words.ndim == 3
    u = (words.astype(np.uint64) >> np.uint64(high_bit + 1 - bits_stored)) & np.uint64((1 << bits_stored) - 1)
    v = u.astype(np.int64)
    if signed:
        v = np.where(u >= np.uint64(1 << (bits_stored - 1)), v - (1 << bits_stored), v)
    if scale is None:
        return v.astype(np.dtype(f"{'i' if signed else 'u'}{words.dtype.itemsize}"))
    scale = np.asarray(scale, dtype=np.float64)
    product = v.astype(np.float64) * scale[None, None, :, 0]            # numpy rounds the product, then the sum: no FMA
    return product + scale[None, None, :, 1]


# ---- packing files ---------------------------------------------------------------------------------------------------------------
def el(group, elem, vr, value, explicit=True, length=None):
    """One element; `length` overrides the length field (UNDEFINED, or a lie for the truncation test)."""
    if isinstance(value, str):
        value = value.encode("ascii")
    if len(value) % 2:
        value += b"\0" if vr in ("UI", "OB", "OW", "UN") else b" "
    n = len(value) if length is None else length
    if not explicit or group == 0xFFFE:
        return struct.pack("<HHI", group, elem, n) + value
    if vr in _LONG:
        return struct.pack("<HH2sHI", group, elem, vr.encode(), 0, n) + value
    return struct.pack("<HH2sH", group, elem, vr.encode(), n) + value


def us(v):
    return struct.pack("<H", v)


def image_elements(rows=3, cols=4, bits=(16, 16, 15, 1), position=(1.0, 2.0, 3.0), orientation=(1, 0, 0, 0, 1, 0), spacing=(0.5, 0.25),
                   slope="2", inter="-1024", series="1.2.3", instance=1, samples=1, frames=None, thickness="2.5", between=None,
                   sop_class="1.2.840.10008.5.1.4.1.1.4"):
    """{tag: (vr, value)} of a slice's header; None values leave the element out."""
    num = lambda vs: "\\".join(repr(float(v)) if not isinstance(v, str) else v for v in vs)
    e = {(0x0008, 0x0016): ("UI", sop_class), (0x0018, 0x0050): ("DS", thickness), (0x0018, 0x0088): ("DS", between),
         (0x0020, 0x000E): ("UI", series), (0x0020, 0x0013): ("IS", None if instance is None else str(instance)),
         (0x0020, 0x0032): ("DS", None if position is None else num(position)),
         (0x0020, 0x0037): ("DS", None if orientation is None else num(orientation)),
         (0x0028, 0x0002): ("US", None if samples is None else us(samples)), (0x0028, 0x0008): ("IS", None if frames is None else str(frames)),
         (0x0028, 0x0010): ("US", None if rows is None else us(rows)), (0x0028, 0x0011): ("US", None if cols is None else us(cols)),
         (0x0028, 0x0030): ("DS", None if spacing is None else num(spacing)),
         (0x0028, 0x0100): ("US", us(bits[0])), (0x0028, 0x0101): ("US", us(bits[1])), (0x0028, 0x0102): ("US", us(bits[2])),
         (0x0028, 0x0103): ("US", us(bits[3])), (0x0028, 0x1052): ("DS", inter), (0x0028, 0x1053): ("DS", slope)}
    return {k: v for k, v in e.items() if v[1] is not None}


def part10(elements, pixels=b"", explicit=True, syntax=None, extra=b"", magic=b"DICM", pixel_tag=(0x7FE0, 0x0010), pixel_length=None,
           pixel_vr="OW"):
    """A part-10 file: preamble, magic, the meta group (explicit VR), the elements in tag order, `extra` (raw bytes of further elements,
    already in the file's VR mode; they sort in front of PixelData) and PixelData.  `pixels` None leaves PixelData out."""
    syntax = syntax or (EXPLICIT if explicit else IMPLICIT)
    meta = el(0x0002, 0x0001, "OB", b"\0\1") + el(0x0002, 0x0002, "UI", "1.2.840.10008.5.1.4.1.1.4") + el(0x0002, 0x0010, "UI", syntax)
    meta = el(0x0002, 0x0000, "UL", struct.pack("<I", len(meta))) + meta
    body = b"".join(el(g, e, vr, v, explicit) for (g, e), (vr, v) in sorted(elements.items()))
    tail = b"" if pixels is None else el(pixel_tag[0], pixel_tag[1], pixel_vr, pixels, explicit, length=pixel_length)
    return b"\0" * 128 + magic + meta + body + extra + tail


def slice_bytes(rows, cols, dtype, k=0, seed=0):
    """(array (rows, cols), its little-endian bytes): seeded words for slice k."""
    a = np.random.default_rng([seed, k]).integers(np.iinfo(dtype).min, int(np.iinfo(dtype).max) + 1, (rows, cols), dtype=np.int64).astype(dtype)
    return a, a.astype(np.dtype(dtype).newbyteorder("<")).tobytes()
