"""`not gpu` side of the DICOM path: the reader (`mmnn_sts_amd.data.dicom`) against files packed here with struct at the published
element layout (tests/_dicom_ref.py shares no code with the package), the series rules (order, geometry, refusals), the synth_dicom
round trip, the host-side refusals of `mmnn_decode_slices`, and the datasets' layout detection and threshold defaults."""
import ctypes
import logging
import os
import struct

import numpy as np
import pytest

from mmnn_sts_amd.data import dicom, synth_dicom, synth_nifti
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _dicom_ref as D


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def _pixels(rows=3, cols=4, dtype="i2", k=0):
    return D.slice_bytes(rows, cols, dtype, k)


# ---- one file ----------------------------------------------------------------------------------------------------------------------
def test_explicit_and_implicit_give_the_same_fields(tmp_path):
    a, raw = _pixels()
    files = [dicom.read_file(_write(tmp_path / f"{int(ex)}.dcm", D.part10(D.image_elements(between="3.0"), raw, explicit=ex))) for ex in (True, False)]
    assert [f.transfer_syntax for f in files] == [D.EXPLICIT, D.IMPLICIT]
    for f in files:
        assert (f.rows, f.columns, f.samples_per_pixel) == (3, 4, 1)
        assert (f.bits_allocated, f.bits_stored, f.high_bit, f.pixel_representation) == (16, 16, 15, 1)
        assert (f.slope, f.inter) == (2.0, -1024.0)
        assert f.pixel_spacing == (0.5, 0.25) and f.position == (1.0, 2.0, 3.0) and f.orientation == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        assert (f.slice_thickness, f.spacing_between_slices, f.instance_number) == (2.5, 3.0, 1.0)
        assert f.series_uid == "1.2.3" and f.sop_class_uid == "1.2.840.10008.5.1.4.1.1.4" and f.number_of_frames is None
        assert f.frame.dtype == np.uint8 and f.frame.tobytes() == raw and not f.frame.flags.writeable
        assert np.array_equal(f.frame.view("<i2").reshape(3, 4), a)


@pytest.mark.parametrize("explicit", [True, False])
def test_sequences_private_and_group_length_elements_are_skipped(tmp_path, explicit):
    e = lambda g, n, vr, v, length=None: D.el(g, n, vr, v, explicit, length)
    decoy = e(0x0028, 0x0010, "US", D.us(999))                                           # Rows inside an item: not the image's
    inner_item = D.el(0xFFFE, 0xE000, None, decoy + D.el(0xFFFE, 0xE00D, None, b""), length=D.UNDEFINED)
    inner = e(0x0008, 0x1140, "SQ", inner_item + D.el(0xFFFE, 0xE0DD, None, b""), length=D.UNDEFINED)
    defined_item = D.el(0xFFFE, 0xE000, None, decoy)
    outer_item = D.el(0xFFFE, 0xE000, None, inner + decoy + D.el(0xFFFE, 0xE00D, None, b""), length=D.UNDEFINED)
    nested = e(0x0008, 0x1115, "SQ", outer_item + defined_item + D.el(0xFFFE, 0xE0DD, None, b""), length=D.UNDEFINED)
    defined_sq = e(0x0008, 0x1111, "SQ", defined_item)
    private = e(0x0029, 0x1010, "UN", b"\x10\x00\x28\x00" * 5)                             # 4-byte length form, bytes that look like a tag
    group_length = e(0x0029, 0x0000, "UL", struct.pack("<I", len(private)))
    empty = e(0x0032, 0x1064, "SQ", b"")
    a, raw = _pixels()
    path = _write(tmp_path / "s.dcm", D.part10(D.image_elements(), raw, explicit, extra=defined_sq + nested + group_length + private + empty))
    f = dicom.read_file(path)
    assert (f.rows, f.columns) == (3, 4) and f.frame.tobytes() == raw


def test_multi_valued_ds_with_padding_and_absent_rescale(tmp_path):
    e = D.image_elements(slope=None, inter=None, spacing=None, position=None)
    e[(0x0028, 0x0030)] = ("DS", " 0.500000 \\0.25\0")
    e[(0x0020, 0x0032)] = ("DS", "-1.5e+01\\ +2 \\3.25 ")
    e[(0x0020, 0x0013)] = ("IS", " 12 ")
    f = dicom.read_file(_write(tmp_path / "p.dcm", D.part10(e, _pixels()[1])))
    assert f.pixel_spacing == (0.5, 0.25) and f.position == (-15.0, 2.0, 3.25) and f.instance_number == 12.0
    assert (f.slope, f.inter) == (1.0, 0.0)


def test_header_only_reads_no_pixel_bytes(tmp_path):
    path = _write(tmp_path / "h.dcm", D.part10(D.image_elements(), _pixels()[1]))
    f = dicom.read_file(path, header_only=True)
    assert f.frame is None and f.has_image and f.pixel_length == 24 and f.pixel_offset == os.path.getsize(path) - 24
    assert dicom.read_series(tmp_path, header_only=True).frames == []


_SYNTAX_REFUSALS = [("1.2.840.10008.1.2.2", "big endian"), ("1.2.840.10008.1.2.1.99", "deflated"), ("1.2.840.10008.1.2.4.50", "compressed"),
                    ("1.2.840.10008.1.2.4.90", "compressed"), ("1.2.840.10008.1.2.5", "compressed"), ("1.2.840.10008.1.2.4.70", "encapsulated")]


@pytest.mark.parametrize("syntax,reason", _SYNTAX_REFUSALS)
def test_refused_transfer_syntaxes(tmp_path, syntax, reason):
    path = _write(tmp_path / "t.dcm", D.part10(D.image_elements(), _pixels()[1], syntax=syntax))
    with pytest.raises(ConfigurationError, match=reason) as err:
        dicom.read_file(path)
    assert path in str(err.value) and syntax in str(err.value)


def test_missing_magic_is_refused(tmp_path):
    path = _write(tmp_path / "m.dcm", D.part10(D.image_elements(), _pixels()[1], magic=b"DICX"))
    with pytest.raises(ConfigurationError, match="magic") as err:
        dicom.read_file(path)
    assert path in str(err.value)
    short = _write(tmp_path / "short.dcm", b"\0" * 40)
    with pytest.raises(ConfigurationError, match="magic"):
        dicom.read_file(short)


_FIELD_REFUSALS = {
    "samples": (dict(samples=3), {}, "SamplesPerPixel 3"),
    "frames": (dict(frames=4), {}, "NumberOfFrames 4"),
    "bits_allocated_12": (dict(bits=(12, 12, 11, 0)), {}, "BitsAllocated 12"),
    "bits_allocated_64": (dict(bits=(64, 16, 15, 0)), {}, "BitsAllocated 64"),
    "bits_stored_0": (dict(bits=(16, 0, 0, 0)), {}, "BitsStored 0"),
    "bits_stored_17": (dict(bits=(16, 17, 15, 0)), {}, "BitsStored 17"),
    "high_bit_low": (dict(bits=(16, 12, 10, 0)), {}, "HighBit 10"),
    "high_bit_high": (dict(bits=(16, 12, 16, 0)), {}, "HighBit 16"),
    "undefined_length": ({}, dict(pixel_length=D.UNDEFINED, pixel_vr="OB"), "undefined length"),
    "truncated": ({}, dict(pixel_length=24, cut=6), "truncated"),
    "short_pixel_data": (dict(rows=4), {}, "truncated"),
    "float_pixel_data": ({}, dict(pixel_tag=(0x7FE0, 0x0008), pixel_vr="OF"), "float pixel data"),
    "double_pixel_data": ({}, dict(pixel_tag=(0x7FE0, 0x0009), pixel_vr="OD"), "double float pixel data"),
}


@pytest.mark.parametrize("name", sorted(_FIELD_REFUSALS))
@pytest.mark.parametrize("explicit", [True, False])
def test_refused_files_name_the_file_and_the_reason(tmp_path, name, explicit):
    fields, packing, reason = _FIELD_REFUSALS[name]
    packing = dict(packing)
    cut = packing.pop("cut", 0)
    data = D.part10(D.image_elements(**fields), _pixels()[1], explicit, **packing)
    path = _write(tmp_path / f"{name}.dcm", data[:len(data) - cut])
    for header_only in (False, True):
        with pytest.raises(ConfigurationError, match=reason) as err:
            dicom.read_file(path, header_only=header_only)
        assert path in str(err.value)


# ---- series --------------------------------------------------------------------------------------------------------------------------
def _series(directory, z=5, rows=3, cols=4, orientation=(1, 0, 0, 0, 1, 0), spacing=(0.5, 0.25), origin=(10.0, -20.0, 5.0), step=2.0,
            names=None, dtype="i2", **fields):
    """z slices along the normal of `orientation`; returns (per-slice arrays in position order, r, c, n)."""
    os.makedirs(directory, exist_ok=True)
    r, c = np.asarray(orientation[:3], dtype=np.float64), np.asarray(orientation[3:], dtype=np.float64)
    n = np.cross(r, c)
    arrays = []
    names = list(names) if names is not None else [f"{k:03d}.dcm" for k in range(z)]
    bits = {"u1": (8, 8, 7, 0), "i2": (16, 16, 15, 1), "u2": (16, 16, 15, 0), "i4": (32, 32, 31, 1)}[dtype]
    for k in range(z):
        a, raw = D.slice_bytes(rows, cols, dtype, k)
        arrays.append(a)
        e = D.image_elements(rows, cols, bits, position=tuple(np.asarray(origin) + k * step * n), orientation=orientation, spacing=spacing,
                             instance=z - k, **fields)
        _write(os.path.join(directory, names[k]), D.part10(e, raw, explicit=bool(k % 2)))
    return arrays, r, c, n


def _volume(series, dtype):
    x, y, z = series.shape
    return np.stack([f.view(np.dtype(dtype).newbyteorder("<")).reshape(y, x).T for f in series.frames], axis=2)


def test_reversed_and_shuffled_names_sort_by_position(tmp_path):
    z = 6
    order = [4, 0, 5, 2, 1, 3]
    for sub, names in (("rev", [f"{z - k:03d}.dcm" for k in range(z)]), ("shuf", [f"img{order[k]}.dcm" for k in range(z)])):
        arrays, *_ = _series(tmp_path / sub, z=z, names=names)
        s = dicom.read_series(tmp_path / sub)
        assert s.shape == (4, 3, z) and (s.bits_allocated, s.bits_stored, s.high_bit, s.signed) == (16, 16, 15, True)
        assert [os.path.basename(p) for p in s.files] == names
        assert np.array_equal(_volume(s, "i2"), np.stack([a.T for a in arrays], axis=2))
        assert s.slopes == [2.0] * z and s.inters == [-1024.0] * z and s.uniform_scale() == (2.0, -1024.0)
        assert s.path == str(tmp_path / sub)


def test_oblique_orientation_against_the_formula_and_the_ras_conversion(tmp_path):
    a, b = 0.3, -0.2
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    ori = tuple(rot[:, 0]) + tuple(rot[:, 1])
    z, step, origin, spacing = 4, 1.75, (3.0, -7.0, 11.0), (0.8, 0.6)
    _, r, c, n = _series(tmp_path / "ob", z=z, orientation=ori, spacing=spacing, origin=origin, step=step, names=[f"{9 - k}.dcm" for k in range(z)])
    s = dicom.read_series(tmp_path / "ob")
    lps = np.eye(4)
    lps[:3, 0], lps[:3, 1] = r * spacing[1], c * spacing[0]                                 # a step in the column index, then in the row index
    p_first, p_last = np.asarray(origin), np.asarray(origin) + (z - 1) * step * n
    lps[:3, 2], lps[:3, 3] = (p_last - p_first) / (z - 1), p_first
    ras = lps.copy()
    ras[:2] *= -1.0
    assert np.allclose(s.affine, ras, rtol=0, atol=1e-12) and s.affine.dtype == np.float64
    # voxel (i, j, k) = (column, row, slice): the last voxel of the last slice lies where the standard's pixel equation puts it
    i, j, k = 3, 2, z - 1
    want = p_last + r * spacing[1] * i + c * spacing[0] * j
    got = s.affine @ np.array([i, j, k, 1.0])
    assert np.allclose(got[:3] * [-1, -1, 1], want, atol=1e-12)


def test_single_slice_third_column(tmp_path):
    for sub, fields, want in (("a", dict(between="3.5"), 3.5), ("b", dict(), 2.5), ("c", dict(thickness=None), 1.0)):
        _series(tmp_path / sub, z=1, **fields)
        s = dicom.read_series(tmp_path / sub)
        assert s.shape == (4, 3, 1) and np.allclose(s.affine[:3, 2], [0, 0, want])           # n = (0, 0, 1) in LPS and in RAS
    e = D.image_elements(position=None, orientation=None, spacing=None)
    _write(tmp_path / "nogeo.dcm", D.part10(e, _pixels()[1]))
    os.makedirs(tmp_path / "ng")
    os.replace(tmp_path / "nogeo.dcm", tmp_path / "ng" / "nogeo.dcm")
    assert dicom.read_series(tmp_path / "ng").affine is None


def test_series_refusals(tmp_path):
    _series(tmp_path / "dup", z=3)
    a, raw = _pixels()
    _write(tmp_path / "dup" / "again.dcm", D.part10(D.image_elements(position=(10.0, -20.0, 7.0)), raw))
    with pytest.raises(ConfigurationError, match="duplicate position") as err:
        dicom.read_series(tmp_path / "dup")
    assert "again.dcm" in str(err.value) and "001.dcm" in str(err.value)
    _series(tmp_path / "rows", z=3)
    _write(tmp_path / "rows" / "tall.dcm", D.part10(D.image_elements(rows=5, position=(10.0, -20.0, 30.0)), D.slice_bytes(5, 4, "i2")[1]))
    with pytest.raises(ConfigurationError, match="differ in Rows") as err:
        dicom.read_series(tmp_path / "rows")
    assert "tall.dcm" in str(err.value) and "000.dcm" in str(err.value)
    _series(tmp_path / "ori", z=3)
    _write(tmp_path / "ori" / "tilt.dcm", D.part10(D.image_elements(orientation=(1, 0, 0, 0, 0.999, 0.04), position=(10.0, -20.0, 30.0)), raw))
    with pytest.raises(ConfigurationError, match="ImageOrientationPatient"):
        dicom.read_series(tmp_path / "ori")
    _series(tmp_path / "nogeo", z=2)
    _write(tmp_path / "nogeo" / "lost.dcm", D.part10(D.image_elements(position=None), raw))
    with pytest.raises(ConfigurationError, match="ImagePositionPatient") as err:
        dicom.read_series(tmp_path / "nogeo")
    assert "lost.dcm" in str(err.value)
    os.makedirs(tmp_path / "two" / "a")
    os.makedirs(tmp_path / "two" / "b")
    with pytest.raises(ConfigurationError, match="2 sub-directories"):
        dicom.read_series(tmp_path / "two")
    os.makedirs(tmp_path / "none")
    _write(tmp_path / "none" / "DICOMDIR", D.part10({}, None))
    _write(tmp_path / "none" / "notes.txt", b"hello")
    with pytest.raises(ConfigurationError, match="no DICOM image files"):
        dicom.read_series(tmp_path / "none")


def test_skipped_files_sub_directory_and_two_series_uids(tmp_path, caplog):
    d = tmp_path / "patient" / "image" / "series_7"
    arrays, *_ = _series(d, z=3)
    _write(d / "DICOMDIR", D.part10({(0x0008, 0x0016): ("UI", "1.2.840.10008.1.3.10")}, None))
    _write(d / "report.txt", b"not DICOM at all, and longer than a preamble" * 8)
    _write(d / ".hidden", b"x")
    a, raw = _pixels()
    _write(d / "other.dcm", D.part10(D.image_elements(series="1.2.9", position=(10.0, -20.0, 99.0)), raw))
    with caplog.at_level(logging.INFO, logger="mmnn_sts_amd.data.dicom"):
        s = dicom.read_series(tmp_path / "patient" / "image")                              # its single sub-directory
    assert s.shape == (4, 3, 3) and s.path == str(d) and np.array_equal(_volume(s, "i2"), np.stack([x.T for x in arrays], axis=2))
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "1.2.9" in warnings[0].getMessage() and "1.2.3" in warnings[0].getMessage()
    assert sum("2 file(s)" in r.getMessage() and "skipped" in r.getMessage() for r in caplog.records) == 1


def test_gap_deviation_warns_once_and_does_not_refuse(tmp_path, caplog):
    _series(tmp_path / "g", z=4)
    a, raw = _pixels()
    _write(tmp_path / "g" / "far.dcm", D.part10(D.image_elements(position=(10.0, -20.0, 5.0 + 9.0)), raw))
    with caplog.at_level(logging.WARNING, logger="mmnn_sts_amd.data.dicom"):
        s = dicom.read_series(tmp_path / "g")
    assert s.shape[2] == 5 and sum("non-uniform" in r.getMessage() for r in caplog.records) == 1
    assert np.allclose(s.affine[:3, 2], [0, 0, 9.0 / 4])


@pytest.mark.parametrize("dtype", ["u1", "i2", "u2", "i4"])
@pytest.mark.parametrize("explicit", [True, False])
def test_synth_dicom_round_trip(tmp_path, dtype, explicit):
    rng = np.random.default_rng(3)
    info = np.iinfo(dtype)
    vol = rng.integers(info.min, int(info.max) + 1, (7, 5, 4), dtype=np.int64).astype(dtype)
    affine = np.eye(4)
    c, s = np.cos(0.2), np.sin(0.2)
    affine[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.diag([0.7, 0.9, 3.1])
    affine[:3, 3] = [-31.25, 12.5, 7.125]
    synth_dicom.write_series(tmp_path / "u", vol, affine, 0.25, -12.5, explicit=explicit, seed=4)
    series = dicom.read_series(tmp_path / "u")
    assert series.shape == vol.shape and np.array_equal(_volume(series, dtype), vol)
    assert (series.bits_allocated, series.bits_stored, series.high_bit, series.signed) == (info.bits, info.bits, info.bits - 1, info.min < 0)
    assert series.uniform_scale() == (0.25, -12.5)
    assert np.abs(series.affine - affine).max() <= 1e-9                                    # decimal strings of at most 16 characters
    assert sorted(os.path.basename(p) for p in series.files) != [os.path.basename(p) for p in series.files]     # names carry no order
    synth_dicom.write_series(tmp_path / "p", vol, affine, 0.25, -12.5, per_slice_scale=True, explicit=explicit)
    series = dicom.read_series(tmp_path / "p")
    assert series.uniform_scale() is None and np.array_equal(_volume(series, dtype), vol)
    assert series.slopes == [0.25 * (1 + (k % 4) / 8) for k in range(4)] and series.inters == [-12.5 - 3.5 * k for k in range(4)]
    assert all(len(synth_dicom.ds(v)) <= 16 for v in (1 / 3, -1e-7 / 3, 123456789.123456789, -79.12345678901234, 0.1, 5.0))
    with pytest.raises(ConfigurationError, match="sheared"):
        synth_dicom.write_series(tmp_path / "sh", vol, affine @ np.array([[1, 0.2, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]))


def test_twelve_stored_bits_round_trip_with_garbage(tmp_path):
    vol = np.random.default_rng(5).integers(-2048, 2048, (6, 5, 3)).astype("i2")
    synth_dicom.write_series(tmp_path / "b", vol, bits_stored=12)
    series = dicom.read_series(tmp_path / "b")
    assert (series.bits_allocated, series.bits_stored, series.high_bit, series.signed) == (16, 12, 11, True)
    words = _volume(series, "u2")
    assert (words >> 12).any() and not np.array_equal(words.view("i2"), vol)                # the unused bits hold garbage
    assert np.array_equal(D.decode_ref(words, 12, 11, True), vol)


# ---- mmnn_decode_slices refuses bad arguments before any launch (no GPU: the pointers are fake and never dereferenced) -----------------
@pytest.fixture(scope="module")
def lib():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


P, O, S = 0x7F0000100000, 0x7F0000900000, 0x7F0000080000        # far apart, 16-byte aligned
_GOOD = dict(x=8, y=4, z=2, bits_allocated=16, bits_stored=12, high_bit=11, is_signed=1, out_type=4)
_BAD_CALLS = {
    "null pixels": ({}, 0, 0, O, "null"), "null out": ({}, P, 0, 0, "null"),
    "zero extent": (dict(y=0), P, 0, O, "non-positive extent"), "negative extent": (dict(z=-3), P, 0, O, "non-positive extent"),
    "2^31 voxels": (dict(x=2048, y=2048, z=512), P, 0, O, "2\\^31"),
    "bits_allocated 12": (dict(bits_allocated=12), P, 0, O, "bits_allocated"), "bits_allocated 64": (dict(bits_allocated=64), P, 0, O, "bits_allocated"),
    "bits_stored 0": (dict(bits_stored=0, high_bit=0), P, 0, O, "bits_stored"), "bits_stored 17": (dict(bits_stored=17, high_bit=15), P, 0, O, "bits_stored"),
    "high_bit below": (dict(high_bit=10), P, 0, O, "high_bit"), "high_bit above": (dict(high_bit=16), P, 0, O, "high_bit"),
    "is_signed 2": (dict(is_signed=2), P, 0, O, "is_signed"),
    "float32 out": (dict(out_type=16), P, 0, O, "out_type"), "unsigned out for signed words": (dict(out_type=512), P, 0, O, "out_type"),
    "wider out": (dict(out_type=8), P, 0, O, "out_type"),
    "scale with an integer out": ({}, P, S, O, "slice_scale"), "float64 out without scale": (dict(out_type=64), P, 0, O, "slice_scale"),
    "pixels misaligned": ({}, P + 1, 0, O, "pixels not aligned"), "integer out misaligned": ({}, P, 0, O + 1, "out not aligned"),
    "float64 out misaligned": (dict(out_type=64), P, S, O + 4, "out not aligned"),
    "out inside pixels": ({}, P, 0, P + 64, "overlap"), "pixels inside float64 out": (dict(out_type=64), O + 128, S, O, "overlap"),
    "out equals pixels": ({}, P, 0, P, "overlap"),
}


@pytest.mark.parametrize("name", sorted(_BAD_CALLS))
def test_decode_slices_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    fields, pixels, scale, out, reason = _BAD_CALLS[name]
    desc = _lib.DecodeSlicesDesc(**dict(_GOOD, **fields))
    assert lib.mmnn_decode_slices(ctypes.byref(desc), pixels or None, scale or None, out or None, None) == 1
    with pytest.raises(ValueError, match=reason):
        _lib.check(1, "mmnn_decode_slices")


def test_decode_slices_refuses_a_null_descriptor(lib):
    assert lib.mmnn_decode_slices(None, P, None, O, None) == 1


# ---- datasets: layout, format key, thresholds ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("trees")
    n = synth_nifti.write_tree(root / "nifti", n_patients=3, seed=11, extent=((8, 12), (8, 12), (4, 6)))
    d = synth_dicom.from_nifti_tree(root / "nifti", root / "dicom")
    return n, d


def _args(**kw):
    import argparse
    return argparse.Namespace(**dict(dict(classification=False, survival=True, images=True, preop=False, postop=False), **kw))


def _parser(tree, **data):
    from mmnn_sts_amd.parser.parser import Parser
    p = Parser()
    p.parseConfig()
    p.config["Data"] = dict({k: tree[k] for k in ("image_loc", "key_loc", "data_loc")}, t1_path="t1", t2_path="t2", **data)
    return p


def test_layout_detection_and_thresholds(trees):
    from mmnn_sts_amd.data import ImageDatasets as I
    n, d = trees
    for tree, layout, threshold in ((n, "nifti", 0.5), (d, "dicom", 128.0)):
        p = _parser(tree)
        ds = p.getDatasets(_args(), p.getImagePath())
        assert ds.layout == ds.t1_dataset.layout == ds.t2_dataset.layout == layout and len(ds) == 3
        assert p.maskResample() == ("auto", threshold)
        p = _parser(tree, mask_threshold=100)
        p.getDatasets(_args(), p.getImagePath())
        assert p.maskResample() == ("auto", 100.0)
    raw = ds[0][0]
    scan, mask = raw.volumes[0]
    assert isinstance(scan, dicom.DicomSeries) and isinstance(mask, dicom.DicomSeries) and scan.shape == mask.shape and len(raw.volumes) == 2
    assert (mask.bits_allocated, mask.signed) == (8, False) and set(np.unique(np.concatenate(mask.frames))) == {0, 255}
    t1 = os.path.join(d["image_loc"], "t1")
    one = I.ImageSurvivalDataset(t1, d["data_loc"], d["key_loc"])
    assert one.layout == "dicom" and len(one[0]) == 3 and I.ImageClassificationDataset(t1, d["data_loc"], d["key_loc"]).layout == "dicom"
    assert one.uids == ds.uids


def test_format_key_and_mixed_trees(trees, tmp_path):
    import shutil
    from mmnn_sts_amd.data import ImageDatasets as I
    n, d = trees
    p = _parser(d, format="DICOM")
    assert p.dataFormat() == "dicom" and p.getDatasets(_args(), p.getImagePath()).layout == "dicom"
    with pytest.raises(ConfigurationError, match="format"):
        _parser(d, format="analyze").getDatasets(_args(), _parser(d).getImagePath())
    p = _parser(d, format="nifti")                                                         # forced: the DICOM tree has no scan* files
    with pytest.raises(ConfigurationError, match="scan"):
        p.getDatasets(_args(), p.getImagePath())
    p = _parser(n, format="dicom")
    with pytest.raises(ConfigurationError, match="image/"):
        p.getDatasets(_args(), p.getImagePath())
    with pytest.raises(ConfigurationError, match="DICOM"):                                 # the NIfTI-layout classes of upstream's DICOM names
        I.ImageSurvivalDataset(os.path.join(n["image_loc"], "t1"), n["data_loc"], n["key_loc"])
    mixed = tmp_path / "mixed"
    shutil.copytree(os.path.join(n["image_loc"], "t1"), mixed)
    victim = sorted(os.listdir(mixed))[1]
    shutil.rmtree(mixed / victim)
    shutil.copytree(os.path.join(d["image_loc"], "t1", victim), mixed / victim)
    with pytest.raises(ConfigurationError, match="mixes the two layouts"):
        I.NiftiSurvivalDataset(str(mixed), n["data_loc"], n["key_loc"])
    with pytest.raises(ConfigurationError, match="slices"):
        I.ImageSurvivalDataset(os.path.join(d["image_loc"], "t1"), d["data_loc"], d["key_loc"], slices=True)


def test_dicom_anonymised_id_is_the_directory_name_when_the_key_has_it(trees, tmp_path):
    import shutil
    from mmnn_sts_amd.data import ImageDatasets as I
    _, d = trees
    tree = tmp_path / "t1"
    shutil.copytree(os.path.join(d["image_loc"], "t1"), tree)
    first = sorted(os.listdir(tree))[0]
    os.rename(tree / first, tree / "WHOLE-NAME-IN-KEY")
    key = tmp_path / "key.csv"
    key.write_text(open(d["key_loc"]).read() + "WHOLE-NAME-IN-KEY,1000\nWHOLE-NAME,4242\n")
    ds = I.ImageSurvivalDataset(str(tree), d["data_loc"], str(key))
    assert ds._uid_of("WHOLE-NAME-IN-KEY") == 1000 and sorted(ds.uids) == [1000, 1007, 1014]


def test_dicom_pair_index_maps():
    from mmnn_sts_amd.data import ingest
    aff = np.diag([0.5, 0.5, 2.0, 1.0])
    mk = lambda shape, a, dcm=True: ingest.DeviceVolume(None, shape, 2, 1.0, 0.0, a, from_dicom=dcm)
    same = ingest.mask_index_map(mk((4, 3, 2), aff), mk((4, 3, 2), aff.copy()))
    assert np.array_equal(same, np.eye(4)[:3])                                             # always a map: the identity on one grid
    assert np.array_equal(ingest.mask_index_map(mk((4, 3, 2), aff), mk((4, 3, 2), aff.copy()), "never"), np.eye(4)[:3])
    assert np.array_equal(ingest.mask_index_map(mk((4, 3, 2), aff), mk((4, 3, 2), None)), np.eye(4)[:3])
    shifted = aff.copy()
    shifted[:3, 3] = [1.0, 0.0, 0.0]
    assert np.allclose(ingest.mask_index_map(mk((4, 3, 2), aff), mk((4, 3, 2), shifted))[:, 3], [-2.0, 0.0, 0.0])
    with pytest.raises(ConfigurationError, match="no geometry"):
        ingest.mask_index_map(mk((4, 3, 2), aff), mk((4, 3, 1), None))
    with pytest.raises(ConfigurationError, match="never"):
        ingest.mask_index_map(mk((4, 3, 2), aff), mk((5, 3, 2), shifted), "never")
    with pytest.raises(ConfigurationError, match="NIfTI mask beside a DICOM scan"):
        ingest.mask_index_map(mk((4, 3, 2), aff), mk((4, 3, 2), aff, dcm=False))
    assert ingest.default_threshold(mk((4, 3, 2), aff)) == 128.0 and ingest.default_threshold(mk((4, 3, 2), aff, dcm=False)) == 0.5
    assert ingest.mask_index_map(mk((4, 3, 2), aff, False), mk((4, 3, 2), aff, False)) is None      # the NIfTI rule is untouched
