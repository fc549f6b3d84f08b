"""`not gpu` side of the RLE Lossless path: synth_dicom's PackBits encoder through the numpy restatement (tests/_dicom_rle_ref.py), the
reader's fields and refusals on encapsulated PixelData packed here with struct, the host-side refusals of `mmnn_rle_expand`, and the
stand-alone host check of the decode core (csrc/rle_core.hpp built with the host compiler under the address and undefined-behaviour
sanitizers), which the hostile streams pass here before tests/test_dicom_rle_gpu.py hands them to the kernel."""
import os
import shutil
import struct

import numpy as np
import pytest

from mmnn_sts_amd.data import dicom, synth_dicom
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _dicom_ref as D
from tests import _dicom_rle_ref as R
from tests import _dicom_stream_harness as H
from tests._dicom_stream_harness import DELIMITER, PAY, PIX, STA, WS, item as _item, write as _write

RLE = "1.2.840.10008.1.2.5"
BITS = {"u1": (8, 8, 7, 0), "i2": (16, 16, 15, 1), "u2": (16, 16, 15, 0), "i4": (32, 32, 31, 1)}


def _rle_file(value, rows=3, cols=4, dtype="i2", **fields):
    """A part-10 file in the RLE syntax whose PixelData (OB, undefined length) holds `value` as it is."""
    return D.part10(D.image_elements(rows, cols, BITS[dtype], **fields), value, syntax=RLE, pixel_vr="OB", pixel_length=D.UNDEFINED)


def _frame(rows=3, cols=4, dtype="i2", k=0):
    a, _ = D.slice_bytes(rows, cols, dtype, k)
    return a, synth_dicom.rle_fragment(a)


# ---- the encoder through the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.volumes()))
def test_encoder_round_trips_through_the_restatement(name):
    vol = R.volumes()[name]
    x, y, z = vol.shape
    bits = vol.dtype.itemsize * 8
    fragments = [synth_dicom.rle_fragment(vol[:, :, k].T) for k in range(z)]
    tables = [R.segment_table(f, bits) for f in fragments]
    assert all(len(f) % 2 == 0 and (t[:, 1] % 2 == 0).all() for f, t in zip(fragments, tables))          # segments padded to even length
    pixels, status = R.rle_expand_ref(fragments, tables, x, y, bits)
    assert not status.any() and np.array_equal(pixels.view(vol.dtype.newbyteorder("<")), vol.transpose(2, 1, 0))


def test_encoder_writes_the_runs_annex_g_asks_for():
    assert synth_dicom.packbits(np.full(130, 7, "u1")) == bytes([129, 7, 255, 7])                    # a repeat of 128, then one of 2
    noise = R.volumes()["257x1x1_noise"].reshape(-1)
    stream = synth_dicom.packbits(noise)
    assert stream == bytes([127]) + noise[:128].tobytes() + bytes([127]) + noise[128:256].tobytes() + bytes([0]) + noise[256:].tobytes()
    assert synth_dicom.packbits(np.array([1, 2, 2, 3], "u1")) == bytes([0, 1, 255, 2, 0, 3])         # runs of 2 become repeat runs
    assert synth_dicom.packbits(np.full(129, 4, "u1")) == bytes([129, 4, 0, 4])
    vol = R.volumes()["130x2x2_constant_rows"]
    fragment = synth_dicom.rle_fragment(vol[:, :, 1].T)                                              # each row on its own: no run crosses a row end
    assert fragment[64:] == bytes([129, 11, 255, 11, 129, 12, 255, 12]) and struct.unpack_from("<16I", fragment) == (1, 64) + (0,) * 14
    with pytest.raises(ConfigurationError, match="explicit"):
        synth_dicom.file_bytes(vol[:, :, 0].T, explicit=False, transfer_syntax="rle")
    with pytest.raises(ConfigurationError, match="transfer_syntax"):
        synth_dicom.file_bytes(vol[:, :, 0].T, transfer_syntax="jpeg")


# ---- one file ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [b"", struct.pack("<I", 0)], ids=["empty_offset_table", "offset_table"])
@pytest.mark.parametrize("dtype", ["u1", "i2", "i4"])
def test_read_file_returns_the_fragment_and_its_segments(tmp_path, table, dtype):
    a, fragment = _frame(dtype=dtype)
    path = _write(tmp_path / "r.dcm", _rle_file(_item(table) + _item(fragment) + DELIMITER, dtype=dtype))
    f = dicom.read_file(path)
    assert f.encoding == "rle" and f.transfer_syntax == RLE and f.has_image and (f.rows, f.columns, f.bits_allocated) == (3, 4, BITS[dtype][0])
    assert f.pixel_length == D.UNDEFINED and f.frame.dtype == np.uint8 and f.frame.tobytes() == fragment
    assert not f.frame.flags.owndata and not f.frame.flags.writeable                                 # a view of the mapped file
    assert f.segments.dtype == np.int64 and np.array_equal(f.segments, R.segment_table(fragment, BITS[dtype][0])) and f.segments[0, 0] == 64
    assert int(f.segments[-1].sum()) == len(fragment)                                               # the last segment reaches the fragment's end
    pixels, status = R.rle_expand_ref([f.frame], [f.segments], 4, 3, BITS[dtype][0])
    assert not status.any() and np.array_equal(pixels[0].view(a.dtype.newbyteorder("<")), a)
    head = dicom.read_file(path, header_only=True)
    assert head.frame is None and head.encoding == "rle" and np.array_equal(head.segments, f.segments) and head.has_image
    native = dicom.read_file(_write(tmp_path / "n.dcm", D.part10(D.image_elements(bits=BITS[dtype]), D.slice_bytes(3, 4, dtype)[1])))
    assert native.encoding == "native" and native.segments is None


def test_read_series_sorts_rle_slices_as_native_ones(tmp_path):
    vol = np.random.default_rng(3).integers(-40, 40, (7, 5, 6)).astype("i2")
    affine = np.diag([0.7, 0.9, 3.1, 1.0])
    affine[:3, 3] = [-31.25, 12.5, 7.125]
    for sub, syntax in (("n", "native"), ("r", "rle")):
        synth_dicom.write_series(tmp_path / sub, vol, affine, 0.25, -12.5, seed=4, transfer_syntax=syntax)
    n, r = dicom.read_series(tmp_path / "n"), dicom.read_series(tmp_path / "r")
    assert (n.encoding, r.encoding) == ("native", "rle") and n.segments == [] and len(r.segments) == len(r.frames) == 6
    assert [os.path.basename(p) for p in n.files] == [os.path.basename(p) for p in r.files] != sorted(os.path.basename(p) for p in r.files)
    assert r.shape == n.shape == vol.shape and np.array_equal(r.affine, n.affine) and r.uniform_scale() == n.uniform_scale() == (0.25, -12.5)
    assert (r.bits_allocated, r.bits_stored, r.high_bit, r.signed) == (n.bits_allocated, n.bits_stored, n.high_bit, n.signed)
    pixels, status = R.rle_expand_ref(r.frames, r.segments, 7, 5, 16)
    assert not status.any() and pixels.tobytes() == b"".join(f.tobytes() for f in n.frames)        # exactly the bytes the uncompressed series holds
    assert sum(f.size for f in r.frames) != sum(f.size for f in n.frames)
    head = dicom.read_series(tmp_path / "r", header_only=True)
    assert head.frames == [] and head.encoding == "rle" and len(head.segments) == 6 and head.shape == vol.shape


def test_a_series_that_mixes_native_and_rle_files_is_refused(tmp_path):
    vol = np.random.default_rng(5).integers(0, 9, (4, 3, 4)).astype("u1")
    synth_dicom.write_series(tmp_path / "m", vol, shuffle_names=False)
    synth_dicom.write_series(tmp_path / "other", vol, shuffle_names=False, transfer_syntax="rle")
    shutil.copyfile(tmp_path / "other" / "0002.dcm", tmp_path / "m" / "0002.dcm")
    with pytest.raises(ConfigurationError, match="mix") as err:
        dicom.read_series(tmp_path / "m")
    assert str(tmp_path / "m" / "0002.dcm") in str(err.value) and RLE in str(err.value)


def _header(count, offsets):
    return struct.pack("<16I", count, *offsets, *([0] * (15 - len(offsets))))


def _refusals(table):
    """{name: (PixelData value, cut, reason)} for a 3 x 4 frame of 16 bits (two segments)."""
    _, good = _frame()
    body = good[64:]
    second = struct.unpack_from("<16I", good)[2]
    bot = _item(table)
    odd = good + b"\0"
    return {
        "no_fragment": (bot + DELIMITER, 0, "0 fragments"),
        "two_fragments": (bot + _item(good) + _item(good) + DELIMITER, 0, "2 fragments"),
        "no_offset_table": (DELIMITER, 0, "Basic Offset Table"),
        "other_item_tag": (bot + _item(good, (0xFFFE, 0xE00D)) + DELIMITER, 0, r"\(FFFE,E00D\).*item"),
        "element_in_place_of_an_item": (bot + _item(good, (0x0008, 0x0018)) + DELIMITER, 0, r"\(0008,0018\).*item"),
        "no_sequence_delimiter": (bot + _item(good), 0, "sequence delimiter"),
        "fragment_past_the_file": (bot + _item(good) + DELIMITER, 8 + 6, "are left in the file"),
        "fragment_of_undefined_length": (bot + _item(good, length=D.UNDEFINED) + DELIMITER, 0, "undefined length"),
        "odd_fragment": (bot + struct.pack("<HHI", 0xFFFE, 0xE000, len(odd)) + odd + DELIMITER, 0, "odd length"),
        "short_fragment": (bot + _item(good[:62]) + DELIMITER, 0, "shorter than its 64-byte header"),
        "one_segment_for_16_bits": (bot + _item(_header(1, [64]) + body) + DELIMITER, 0, "counts 1 segments"),
        "three_segments_for_16_bits": (bot + _item(_header(3, [64, second, second + 2]) + body) + DELIMITER, 0, "counts 3 segments"),
        "first_offset_66": (bot + _item(_header(2, [66, second]) + body) + DELIMITER, 0, "first RLE segment starts at byte 66"),
        "first_offset_0": (bot + _item(_header(2, [0, second]) + body) + DELIMITER, 0, "first RLE segment starts at byte 0"),
        "offsets_descend": (bot + _item(_header(2, [64, 60]) + body) + DELIMITER, 0, "do not ascend"),
        "offsets_equal": (bot + _item(_header(2, [64, 64]) + body) + DELIMITER, 0, "do not ascend"),
        "offset_past_the_fragment": (bot + _item(_header(2, [64, len(good) + 2]) + body) + DELIMITER, 0, "do not ascend strictly inside"),
        "offset_behind_the_used_ones": (bot + _item(_header(2, [64, second, 0, 0, second + 2]) + body) + DELIMITER, 0, "non-zero offset behind"),
    }


@pytest.mark.parametrize("table", [b"", struct.pack("<I", 0)], ids=["empty_offset_table", "offset_table"])
@pytest.mark.parametrize("name", sorted(_refusals(b"")))
def test_refused_rle_files_name_the_file_and_the_reason(tmp_path, name, table):
    value, cut, reason = _refusals(table)[name]
    data = _rle_file(value)
    path = _write(tmp_path / f"{name}.dcm", data[:len(data) - cut])
    for header_only in (False, True):
        with pytest.raises(ConfigurationError, match=reason) as err:
            dicom.read_file(path, header_only=header_only)
        assert path in str(err.value)


def test_defined_length_pixel_data_in_the_rle_syntax_is_refused(tmp_path):
    path = _write(tmp_path / "d.dcm", D.part10(D.image_elements(), D.slice_bytes(3, 4, "i2")[1], syntax=RLE))
    with pytest.raises(ConfigurationError, match="compressed and needs encapsulated PixelData of undefined length") as err:
        dicom.read_file(path)
    assert path in str(err.value) and RLE in str(err.value)
    for explicit in (True, False):              # the uncompressed syntaxes keep refusing encapsulated PixelData
        path = _write(tmp_path / f"u{int(explicit)}.dcm", D.part10(D.image_elements(), b"", explicit, pixel_vr="OB", pixel_length=D.UNDEFINED))
        with pytest.raises(ConfigurationError, match="undefined length"):
            dicom.read_file(path)


# ---- mmnn_rle_expand refuses bad arguments before any launch (no GPU: the pointers are fake and never dereferenced) --------------------
@pytest.fixture(scope="module")
def lib():
    return H.built_lib()


_BAD_CALLS = H.bad_calls("segments", too_deep=64)


@pytest.mark.parametrize("name", sorted(_BAD_CALLS))
def test_rle_expand_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    H.assert_refused(lib, "mmnn_rle_expand", _lib.RleDesc, *_BAD_CALLS[name])


def test_rle_expand_refuses_a_null_descriptor(lib):
    assert lib.mmnn_rle_expand(None, PAY, H.TAB, PIX, STA, WS, None) == 1


def test_rle_workspace_bytes_is_monotone_and_refuses_bad_extents(lib):
    from mmnn_sts_amd import _lib
    size = lambda x, y, z, bits: _lib.count("mmnn_rle_workspace_bytes", x, y, z, bits)
    assert _lib.RLE_CHUNK >= 256 and _lib.RLE_CHUNK % 16 == 0
    for bits in (8, 16, 32):
        sizes = [size(*e, bits) for e in ((1, 1, 1), (5, 3, 2), (64, 64, 3), (512, 512, 48), (512, 512, 96), (1024, 512, 96))]
        assert sizes == sorted(sizes) and sizes[0] > 0
    assert size(512, 512, 48, 8) <= size(512, 512, 48, 16) <= size(512, 512, 48, 32)
    assert size(512, 512, 48, 16) >= 512 * 512 * 48 * 2                                              # the byte planes before they meet
    for bad in ((0, 4, 4, 16), (4, -1, 4, 16), (4, 4, 0, 8), (2048, 2048, 512, 8), (4, 4, 4, 12), (4, 4, 4, 0)):
        assert lib.mmnn_rle_workspace_bytes(*bad) < 0
        with pytest.raises(ValueError, match="rle_workspace_bytes"):
            size(*bad)


# ---- the decode core on the host, under the sanitizers ---------------------------------------------------------------------------------
def host_check_cases():
    """[(name, x, y, z, bits, payload, table)]: every stream the GPU test gives the kernel -- the encoder's, the hand-built, the malformed,
    and tables that lie about where a segment is."""
    from mmnn_sts_amd import _lib
    cases = []
    for name, vol in R.volumes().items():
        x, y, z = vol.shape
        bits = vol.dtype.itemsize * 8
        fragments = [synth_dicom.rle_fragment(vol[:, :, k].T) for k in range(z)]
        cases.append((name, x, y, z, bits, [bytes(f) for f in fragments], [R.segment_table(f, bits) for f in fragments]))
    for name, (x, y, bits, streams) in R.hand_streams(_lib.RLE_CHUNK).items():
        fragment, table = R.rle_fragment(streams)
        cases.append((name, x, y, 1, bits, [fragment], [table]))
    for name in R.malformed_streams():
        for bits in (8, 16):
            fragments, tables, x, y, _ = R.malformed_frames(name, bits)
            cases.append((f"{name}_{bits}", x, y, 3, bits, fragments, tables))
    fragments, tables, x, y, bits = R.malformed_frames("cut_mid_literal", 16)
    for name, lie in (("offset_far_past_the_payload", (1 << 40, 50)), ("negative_offset", (-300, 200)), ("length_past_the_payload", (64, 1 << 40)),
                      ("negative_length", (64, -5)), ("offset_at_the_last_byte", (len(fragments[2]) - 1, 99))):
        t = [np.array(t) for t in tables]
        t[2][0] = lie
        cases.append((name, x, y, 3, bits, fragments, t))
    return cases


def test_decode_core_on_the_host_under_sanitizers(tmp_path):
    cases = host_check_cases()
    packed = []
    for name, x, y, z, bits, fragments, tables in cases:
        payload, table = R.pack_payload(fragments, tables)
        packed.append((x, y, z, bits, payload, table))
    results = H.run_host_check(tmp_path, "rle_core_check", packed, R.RECORD)
    for (name, x, y, z, bits, fragments, tables), (_, _, _, _, payload, table), got in zip(cases, packed, results):
        want = R.rle_expand_ref([payload] * z, list(table), x, y, bits)           # offsets into the payload, clamped alike
        _, status = H.assert_equals_restatement(name, got, want, who="host check")
        if name.split("_")[0] in ("cut", "noops", "zero", "ends") and not name.startswith("noops_straddles"):
            assert status.tolist() == [0, 1, 0], name
