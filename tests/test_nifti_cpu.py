"""mmnn_sts_amd.data.nifti against the published NIfTI-1 layout.  The reader is fed files this test assembles with struct.pack at the
published offsets (tests/_ingest_ref.py: pack_nifti); the writer's bytes are parsed by struct.unpack at the same offsets.  Reader and
writer are never checked against each other alone."""
import gzip

import numpy as np
import pytest

from mmnn_sts_amd.data import nifti
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests._ingest_ref import NP_OF_CODE, fdata, pack_nifti, parse_nifti, read_nifti_file


def _ramp(code, shape=(5, 3, 2)):
    n = int(np.prod(shape))
    return (np.arange(n) + 1).reshape(shape, order="F").astype(NP_OF_CODE[code])       # x fastest: voxel (x, y, z) = 1 + x + 5 y + 15 z


def _put(tmp_path, name, data):
    p = tmp_path / name
    if name.endswith(".gz"):
        with gzip.open(p, "wb") as f:
            f.write(data)
    else:
        p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("byteorder", ["<", ">"])
@pytest.mark.parametrize("code", sorted(NP_OF_CODE))
def test_reader_every_type_both_byte_orders(tmp_path, code, byteorder):
    raw = _ramp(code)
    img = nifti.read(_put(tmp_path, "v.nii", pack_nifti(raw, code, 2.0, -1.0, byteorder)))
    assert img.datatype == code and img.raw.dtype == np.dtype(NP_OF_CODE[code]) and img.raw.dtype.isnative
    assert img.shape == (5, 3, 2) and np.array_equal(img.raw, raw)
    assert img.raw[1, 0, 0] == 2 and img.raw[0, 1, 0] == 6 and img.raw[0, 0, 1] == 16          # x fastest
    assert img.raw.flags.f_contiguous                                                           # the file's memory order is kept
    assert (img.slope, img.inter) == (2.0, -1.0)
    assert img.get_fdata().dtype == np.float64 and np.array_equal(img.get_fdata(), fdata(raw, 2.0, -1.0))


def test_reader_gz_and_plain_agree(tmp_path):
    data = pack_nifti(_ramp(4), 4, 0.5, 3.0)
    a, b = nifti.read(_put(tmp_path, "a.nii", data)), nifti.read(_put(tmp_path, "b.nii.gz", data))
    assert np.array_equal(a.raw, b.raw) and (a.slope, a.inter) == (b.slope, b.inter) == (0.5, 3.0)


@pytest.mark.parametrize("slope", [0.0, float("nan"), float("inf")])
def test_reader_degenerate_slope_means_unscaled(tmp_path, slope):
    raw = _ramp(4)
    img = nifti.read(_put(tmp_path, "v.nii", pack_nifti(raw, 4, slope, 7.0)))
    assert img.scaling() is None
    assert np.array_equal(img.get_fdata(), raw.astype(np.float64))


def test_reader_4d_with_trailing_one(tmp_path):
    raw = _ramp(16)
    img = nifti.read(_put(tmp_path, "v.nii", pack_nifti(raw, 16, dim=[4, 5, 3, 2, 1])))
    assert img.shape == (5, 3, 2) and np.array_equal(img.raw, raw)


@pytest.mark.parametrize("code", [128, 32])
def test_reader_refuses_rgb_and_complex(tmp_path, code):
    data = pack_nifti(np.zeros((5, 3, 2), dtype="u1"), code)
    with pytest.raises(ConfigurationError, match=str(code)):
        nifti.read(_put(tmp_path, "v.nii", data))


def test_reader_refuses_header_pair_magic(tmp_path):
    with pytest.raises(ConfigurationError, match="hdr"):
        nifti.read(_put(tmp_path, "v.nii", pack_nifti(_ramp(4), 4, magic=b"ni1\0")))


def test_reader_refuses_truncated_data(tmp_path):
    with pytest.raises(ConfigurationError, match="truncated"):
        nifti.read(_put(tmp_path, "v.nii", pack_nifti(_ramp(4), 4, truncate=3)))


def test_reader_refuses_foreign_file(tmp_path):
    with pytest.raises(ConfigurationError, match="sizeof_hdr"):
        nifti.read(_put(tmp_path, "v.nii", b"\x01" * 400))


@pytest.mark.parametrize("dtype,code", [("float32", 16), ("int16", 4), ("uint8", 2)])
@pytest.mark.parametrize("name", ["w.nii", "w.nii.gz"])
def test_writer_bytes_at_the_published_offsets(tmp_path, dtype, code, name):
    rng = np.random.default_rng(3)
    a = (rng.random((6, 4, 3)) * 100).astype(dtype)
    path = nifti.write(tmp_path / name, a)
    h = read_nifti_file(path)
    assert h["sizeof_hdr"] == 348 and h["magic"] == b"n+1\0" and h["vox_offset"] == 352.0
    assert h["dim"][:4] == (3, 6, 4, 3) and h["datatype"] == code and h["bitpix"] == a.dtype.itemsize * 8
    assert h["sform_code"] > 0 and np.array_equal(h["srow"], np.eye(4)[:3])                    # identity affine
    assert np.array_equal(h["data"], a)
    back = nifti.read(path)                                                                    # write -> read round trip, exact
    assert back.raw.dtype == a.dtype and np.array_equal(back.raw, a) and back.datatype == code


def test_writer_layout_independent_and_refusals(tmp_path):
    a = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    p1, p2 = nifti.write(tmp_path / "c.nii", a), nifti.write(tmp_path / "f.nii", np.asfortranarray(a))
    assert open(p1, "rb").read() == open(p2, "rb").read()
    assert parse_nifti(open(p1, "rb").read())["data"][1, 2, 3] == a[1, 2, 3]
    with pytest.raises(ConfigurationError):
        nifti.write(tmp_path / "x.nii", a.astype(np.complex64))
