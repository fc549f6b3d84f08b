"""`not gpu` side of the JPEG Lossless path: three entropy-coded streams typed in with their derivation, synth_dicom's encoder through the
restatement (tests/_dicom_jpegll_ref.py), the reader's fields and refusals on JPEG streams packed here with struct, the host-side
refusals of `mmnn_jpegll_decode`, and the stand-alone host check of the positional core (csrc/jpegll_core.hpp built with the host
compiler under the address and undefined-behaviour sanitizers), which the hostile streams pass here before
tests/test_dicom_jpegll_gpu.py hands them to the kernel."""
import os
import shutil
import struct

import numpy as np
import pytest

from mmnn_sts_amd.data import dicom, synth_dicom
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _dicom_jpegll_ref as R
from tests import _dicom_ref as D
from tests import _dicom_stream_harness as H
from tests._dicom_stream_harness import DELIMITER, PAY, PIX, STA, WS, item as _item, write as _write

SV1, P14 = "1.2.840.10008.1.2.4.70", "1.2.840.10008.1.2.4.57"
BITS = {"u1": (8, 8, 7, 0), "i2": (16, 16, 15, 1), "u2": (16, 16, 15, 0), "i4": (32, 32, 31, 1)}


# ---- typed-in streams ------------------------------------------------------------------------------------------------------------------
# Table K.3: SSSS 0 is 00, 1..5 are 010 011 100 101 110, 6 is 1110, 7 is 11110, 8 is 111110 ...; the extended table goes on with one
# code per length, so SSSS 16 is the 14-bit code 11111111111110.  A difference d > 0 is followed by its SSSS bits, d < 0 by those of
# d + 2^SSSS - 1.
TYPED_IN = {
    # [[130,129],[126,126]] at P = 8: predictions 128, 130 (left), 130 (above), 126 (left); differences 2, -1, -4, 0;
    # 011 10 | 010 0 | 100 011 | 00 + 1111111 -> 01110010 01000110 01111111
    "k3_2x2": (R.K3, 8, [[130, 129], [126, 126]], "72 46 7F"),
    # [[255,0,255],[0,255,0]] at P = 8: differences 127, -255, 255, -255 (from the 255 above), 255, -255;
    # 127: 11110 1111111; -255: 111110 00000000; 255: 111110 11111111 -> three FF bytes, each stuffed
    "k3_3x2_stuffed": (R.K3, 8, [[255, 0, 255], [0, 255, 0]], "F7 FF 00 80 3E FF 00 F8 03 EF FF 00 80 3F"),
    # [[0, 32768]] at P = 16: the prediction 32768 gives 0 - 32768 = 32768 modulo 2^16, then 32768 - 0: SSSS 16 twice, no extra bits;
    # 11111111 111110 11 11111111 1110 + 1111 -> FF FB FF EF, two of them stuffed
    "extended_ssss16": (R.EXTENDED, 16, [[0, 32768]], "FF 00 FB FF 00 EF"),
}


@pytest.mark.parametrize("name", sorted(TYPED_IN))
def test_typed_in_streams(name):
    table, precision, frame, data = TYPED_IN[name]
    frame, data = np.array(frame), bytes.fromhex(data)
    words, status = R.decode_frame(data + b"\xff\xd9", table[0], table[1], precision, frame.shape[1], frame.shape[0], 16)
    assert status == 0 and np.array_equal(words, frame)
    assert R.encode(frame, precision, table) == data
    dtype = "u1" if precision == 8 else "u2"
    fragment = synth_dicom.jpeg_lossless_fragment(frame.astype(dtype), table=table)
    at, p, t = R.scan_of(fragment)
    assert (p, t) == (precision, table) and fragment[:2] == b"\xff\xd8" and fragment[at:] in (data + b"\xff\xd9", data + b"\xff\xd9\0")
    if table == R.K3:                           # the default table extends K.3: the same codes for the categories K.3 has
        default = synth_dicom.jpeg_lossless_fragment(frame.astype(dtype))
        assert default[R.scan_of(default)[0]:].startswith(data + b"\xff\xd9") and R.scan_of(default)[2] == R.EXTENDED


def test_default_table_is_k3_extended():
    bits, values = synth_dicom.JPEG_DEFAULT_TABLE
    assert (bits, values) == R.EXTENDED and sum(bits) == 17 and sum(c << (16 - l) for l, c in enumerate(bits, 1)) == (1 << 16) - 4
    assert [l for l, _, _ in R.code_table(bits, values)][:12] == [l for l, _, _ in R.code_table(*R.K3)]


# ---- the encoder through the restatement ---------------------------------------------------------------------------------------------
def _fragments(vol, bits_stored, table="default"):
    return [synth_dicom.jpeg_lossless_fragment(vol[:, :, k].T, bits_stored, table) for k in range(vol.shape[2])]


@pytest.mark.parametrize("table", ["default", "frame"])
@pytest.mark.parametrize("name", sorted(R.volumes()))
def test_encoder_round_trips_through_the_restatement(name, table):
    vol, bits_stored = R.volumes()[name]
    x, y, z = vol.shape
    fragments = _fragments(vol, bits_stored, table)
    assert all(len(f) % 2 == 0 and f.rstrip(b"\0").endswith(b"\xff\xd9") for f in fragments)
    payload, records = R.pack_fragments(fragments)
    assert (records["precision"] == R.precision_of(vol, bits_stored)).all()
    pixels, status = R.decode_ref(payload, records, x, y, vol.dtype.itemsize * 8)
    assert not status.any() and np.array_equal(pixels.view(vol.dtype.newbyteorder("<")), vol.transpose(2, 1, 0))
    if table == "default":                      # the two encoders agree bit for bit
        for k, f in enumerate(fragments):
            words = vol[:, :, k].T.view(f"u{vol.dtype.itemsize}")
            assert f[R.scan_of(f)[0]:].rstrip(b"\0")[:-2] == R.encode(words, R.precision_of(vol, bits_stored))


def test_frame_tables_reach_code_lengths_1_and_16():
    constant = synth_dicom.jpeg_lossless_fragment(np.full((4, 4), 128, "u1"), table="frame")
    assert R.scan_of(constant)[2] == ((1,) + (0,) * 15, (0,))                                        # SSSS 0 alone: the code 0
    counts = [v for v in range(17) for _ in range(1 << v)]
    bits, values = synth_dicom.frame_table(np.array(counts))
    assert bits[15] >= 1 and sorted(values) == list(range(17)) and sum(c << (16 - l) for l, c in enumerate(bits, 1)) < 1 << 16
    noise = R.volumes()["64x64x2_i2_noise"][0]
    assert 2600 < synth_dicom.jpeg_lossless_fragment(noise[:, :, 0].T).count(b"\xff\x00") < 2800      # heavy stuffing, several chunks
    with pytest.raises(ConfigurationError, match="transfer_syntax"):
        synth_dicom.file_bytes(noise[:, :, 0].T, transfer_syntax="jpeg")
    with pytest.raises(ConfigurationError, match="16 bits"):
        synth_dicom.file_bytes(noise[:, :, 0].T.astype("i4"), transfer_syntax="jpeg-lossless")
    with pytest.raises(ConfigurationError, match="explicit"):
        synth_dicom.file_bytes(noise[:, :, 0].T, explicit=False, transfer_syntax="jpeg-lossless")


# ---- one file ------------------------------------------------------------------------------------------------------------------------
SOI, EOI = b"\xff\xd8", b"\xff\xd9"


def _segment(marker, body, length=None):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2 if length is None else length) + body


def _dht(table=R.EXTENDED, tc=0, th=0):
    return bytes([tc << 4 | th]) + bytes(table[0]) + bytes(table[1])


def _sof(p=16, lines=3, samples=4, nf=1, marker=0xC3):
    return _segment(marker, struct.pack(">BHHB", p, lines, samples, nf) + bytes([1, 0x11, 0]) * nf)


def _sos(ns=1, td=0, ss=1, al=0):
    return _segment(0xDA, bytes([ns]) + bytes([1, td << 4]) * ns + bytes([ss, 0, al]))


def _stream(*segments, data=b"\x12\x34"):
    return SOI + b"".join(segments) + data + EOI


def _good(**sof):
    return _stream(_segment(0xC4, _dht()), _sof(**sof), _sos())


def _jpeg_file(value, rows=3, cols=4, dtype="i2", syntax=SV1, bits=None, **fields):
    """A part-10 file in a JPEG Lossless syntax whose PixelData (OB, undefined length) holds `value` as it is."""
    return D.part10(D.image_elements(rows, cols, bits or BITS[dtype], **fields), value, syntax=syntax, pixel_vr="OB", pixel_length=D.UNDEFINED)


def _one(stream, table=b""):
    return _item(table) + _item(stream + b"\0" * (len(stream) % 2)) + DELIMITER


@pytest.mark.parametrize("table", [b"", struct.pack("<I", 0)], ids=["empty_offset_table", "offset_table"])
@pytest.mark.parametrize("dtype,syntax", [("u1", SV1), ("i2", SV1), ("u2", P14)])
def test_read_file_returns_the_fragment_and_its_scan(tmp_path, table, dtype, syntax):
    a, _ = D.slice_bytes(3, 4, dtype)
    fragment = synth_dicom.jpeg_lossless_fragment(a)
    path = _write(tmp_path / "j.dcm", _jpeg_file(_item(table) + _item(fragment) + DELIMITER, dtype=dtype, syntax=syntax))
    f = dicom.read_file(path)
    assert f.encoding == "jpeg-lossless" == dicom.JPEGLL and f.transfer_syntax == syntax and f.has_image and f.segments is None
    assert (f.rows, f.columns, f.bits_allocated) == (3, 4, BITS[dtype][0]) and f.pixel_length == D.UNDEFINED
    assert f.frame.dtype == np.uint8 and f.frame.tobytes() == fragment
    assert not f.frame.flags.owndata and not f.frame.flags.writeable                                 # a view of the mapped file
    at, precision, (bits, values) = R.scan_of(fragment)
    j = f.jpeg
    assert (j.precision, j.lines, j.samples, j.offset, j.length) == (precision, 3, 4, at, len(fragment) - at) and precision == BITS[dtype][0]
    assert j.bits.dtype == np.uint8 and tuple(j.bits) == bits and tuple(j.huffval) == values and len(j.huffval) == 17
    words, status = R.decode_frame(f.frame[j.offset:j.offset + j.length], j.bits, j.huffval, j.precision, 4, 3, BITS[dtype][0])
    assert status == 0 and np.array_equal(words.view(a.dtype.newbyteorder("<")), a)
    head = dicom.read_file(path, header_only=True)
    assert head.frame is None and head.encoding == "jpeg-lossless" and head.jpeg.offset == j.offset and head.has_image
    native = dicom.read_file(_write(tmp_path / "n.dcm", D.part10(D.image_elements(bits=BITS[dtype]), D.slice_bytes(3, 4, dtype)[1])))
    assert native.encoding == "native" and native.jpeg is None


def test_skipped_segments_and_the_selected_table(tmp_path):
    other = ((0, 3) + (0,) * 14, (0, 1, 2))
    stream = _stream(_segment(0xE0, b"JFIF\0" + bytes(9)), _segment(0xFE, b"a comment \xff\xda inside"), _segment(0xC4, _dht(R.K3, th=0) + _dht(other, th=3)),
                     _segment(0xDD, struct.pack(">H", 0)), b"\xff", _segment(0xC4, _dht(R.EXTENDED, th=1)), _sof(p=12), _sos(td=3), data=b"\xaa\xbb\xcc")
    f = dicom.read_file(_write(tmp_path / "s.dcm", _jpeg_file(_one(stream), bits=(16, 12, 11, 0))))
    assert tuple(f.jpeg.bits) == other[0] and tuple(f.jpeg.huffval) == other[1] and f.jpeg.precision == 12
    assert f.frame[f.jpeg.offset:].tobytes().startswith(b"\xaa\xbb\xcc\xff\xd9") and f.jpeg.offset + f.jpeg.length == f.frame.size


def test_read_series_sorts_jpeg_slices_as_native_ones(tmp_path):
    vol = np.random.default_rng(3).integers(-40, 40, (7, 5, 6)).astype("i2")
    affine = np.diag([0.7, 0.9, 3.1, 1.0])
    affine[:3, 3] = [-31.25, 12.5, 7.125]
    for sub, syntax in (("n", "native"), ("j", "jpeg-lossless")):
        synth_dicom.write_series(tmp_path / sub, vol, affine, 0.25, -12.5, seed=4, transfer_syntax=syntax)
    n, j = dicom.read_series(tmp_path / "n"), dicom.read_series(tmp_path / "j")
    assert (n.encoding, j.encoding) == ("native", "jpeg-lossless") and n.jpeg == [] and j.segments == [] and len(j.jpeg) == len(j.frames) == 6
    assert [os.path.basename(p) for p in n.files] == [os.path.basename(p) for p in j.files] != sorted(os.path.basename(p) for p in j.files)
    assert j.shape == n.shape == vol.shape and np.array_equal(j.affine, n.affine) and j.uniform_scale() == n.uniform_scale() == (0.25, -12.5)
    assert (j.bits_allocated, j.bits_stored, j.high_bit, j.signed) == (n.bits_allocated, n.bits_stored, n.high_bit, n.signed)
    payload, records = R.pack_fragments([f.tobytes() for f in j.frames])
    pixels, status = R.decode_ref(payload, records, 7, 5, 16)
    assert not status.any() and pixels.tobytes() == b"".join(f.tobytes() for f in n.frames)        # exactly the bytes the uncompressed series holds
    assert sum(s.length for s in j.jpeg) < sum(f.size for f in n.frames)                             # (the entropy-coded data; the markers outweigh it at 7 x 5)
    head = dicom.read_series(tmp_path / "j", header_only=True)
    assert head.frames == [] and head.encoding == "jpeg-lossless" and len(head.jpeg) == 6 and head.shape == vol.shape


@pytest.mark.parametrize("pair", [("native", "jpeg-lossless"), ("rle", "jpeg-lossless")])
def test_a_series_that_mixes_encodings_is_refused(tmp_path, pair):
    vol = np.random.default_rng(5).integers(0, 9, (4, 3, 4)).astype("u1")
    synth_dicom.write_series(tmp_path / "m", vol, shuffle_names=False, transfer_syntax=pair[0])
    synth_dicom.write_series(tmp_path / "other", vol, shuffle_names=False, transfer_syntax=pair[1])
    shutil.copyfile(tmp_path / "other" / "0002.dcm", tmp_path / "m" / "0002.dcm")
    with pytest.raises(ConfigurationError, match="mix") as err:
        dicom.read_series(tmp_path / "m")
    assert str(tmp_path / "m" / "0002.dcm") in str(err.value) and SV1 in str(err.value) and "JPEG lossless" in str(err.value)


# {name: (PixelData value, reason, keywords of _jpeg_file)} for a 3 x 4 frame of 16 bits
_REFUSALS = {
    "sof1": (_one(_stream(_segment(0xC4, _dht()), _sof(marker=0xC1), _sos())), r"SOF1 \(FFC1\).*only SOF3", {}),
    "sof0_baseline": (_one(_stream(_segment(0xC4, _dht()), _sof(marker=0xC0), _sos())), r"SOF0 \(FFC0\).*only SOF3", {}),
    "three_components": (_one(_stream(_segment(0xC4, _dht()), _sof(nf=3), _sos())), r"3 components \(Nf\)", {}),
    "two_scan_components": (_one(_stream(_segment(0xC4, _dht()), _sof(), _sos(ns=2))), r"2 components \(Ns\)", {}),
    "predictor_4": (_one(_stream(_segment(0xC4, _dht()), _sof(), _sos(ss=4))), "predictor 4.*predictors 2-7 are out of scope", {}),
    "predictor_7_in_process_14": (_one(_stream(_segment(0xC4, _dht()), _sof(), _sos(ss=7))), "predictors 2-7 are out of scope", dict(syntax=P14)),
    "predictor_0": (_one(_stream(_segment(0xC4, _dht()), _sof(), _sos(ss=0))), "predictor 0", {}),
    "point_transform": (_one(_stream(_segment(0xC4, _dht()), _sof(), _sos(al=2))), r"point transform of 2 \(Al\)", {}),
    "restart_interval": (_one(_stream(_segment(0xC4, _dht()), _segment(0xDD, struct.pack(">H", 8)), _sof(), _sos())), "restart interval of 8", {}),
    "dnl": (_one(_stream(_segment(0xC4, _dht()), _sof(), _segment(0xDC, struct.pack(">H", 3)), _sos())), "DNL", {}),
    "precision_1": (_one(_good(p=1)), r"precision 1 \(P\) outside 2..16", {}),
    "precision_17": (_one(_good(p=17)), r"precision 17 \(P\) outside 2..16", {}),
    "precision_above_bits_allocated": (_one(_good(p=12)), r"precision 12 \(P\) outside BitsStored 8 .. BitsAllocated 8", dict(dtype="u1")),
    "precision_below_bits_stored": (_one(_good(p=12)), r"precision 12 \(P\) outside BitsStored 16 .. BitsAllocated 16", {}),
    "bits_allocated_32": (_one(_good()), "BitsAllocated 32", dict(dtype="i4")),
    "lines_differ": (_one(_good(lines=4)), "4 lines of 4 samples.*3 x 4", {}),
    "samples_differ": (_one(_good(samples=5)), "3 lines of 5 samples.*3 x 4", {}),
    "no_dht_for_the_selected_table": (_one(_stream(_segment(0xC4, _dht()), _sof(), _sos(td=1))), r"selects Huffman table 1.*no DHT", {}),
    "no_dht_at_all": (_one(_stream(_sof(), _sos())), "no DHT", {}),
    "table_class_1": (_one(_stream(_segment(0xC4, _dht(tc=1)), _sof(), _sos())), "class 1", {}),
    "bits_sum_18": (_one(_stream(_segment(0xC4, _dht(((0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0), tuple(range(17)) + (0,)))), _sof(), _sos())), "counts 18 codes", {}),
    "huffval_17": (_one(_stream(_segment(0xC4, _dht((R.EXTENDED[0], tuple(range(16)) + (17,)))), _sof(), _sos())), "holds the value 17", {}),
    "repeated_values": (_one(_stream(_segment(0xC4, _dht((R.EXTENDED[0], tuple(range(16)) + (3,)))), _sof(), _sos())), "repeated values", {}),
    "over_subscribed": (_one(_stream(_segment(0xC4, _dht(((3,) + (0,) * 15, (0, 1, 2)))), _sof(), _sos())), "over-subscribed", {}),
    "segment_past_the_fragment": (_one(_stream(_segment(0xC4, _dht(), length=500), _sof(), _sos())), "declares 500 bytes and runs past the fragment", {}),
    "table_past_its_segment": (_one(_stream(_segment(0xC4, _dht()[:20]), _sof(), _sos())), "run past its DHT segment", {}),
    "no_sos": (_one(SOI + _segment(0xC4, _dht()) + _sof()), "no SOS found", {}),
    "no_soi": (_one(_good()[2:]), "does not start with SOI", {}),
    "sos_without_sof": (_one(_stream(_segment(0xC4, _dht()), _sos())), "without a frame header", {}),
    "eoi_in_front_of_sos": (_one(SOI + EOI + _good()[2:]), "FFD9 at byte 2.*where a marker segment was expected", {}),
    "two_fragments": (_item(b"") + _item(_good()) + _item(_good()) + DELIMITER, "2 fragments", {}),
    "no_fragment": (_item(b"") + DELIMITER, "0 fragments", {}),
    "no_sequence_delimiter": (_item(b"") + _item(_good()), "sequence delimiter", {}),
}


@pytest.mark.parametrize("name", sorted(_REFUSALS))
def test_refused_jpeg_files_name_the_file_and_the_reason(tmp_path, name):
    value, reason, fields = _REFUSALS[name]
    path = _write(tmp_path / f"{name}.dcm", _jpeg_file(value, **fields))
    for header_only in (False, True):
        with pytest.raises(ConfigurationError, match=reason) as err:
            dicom.read_file(path, header_only=header_only)
        assert path in str(err.value)


def test_the_sound_stream_of_the_refusals_is_read(tmp_path):
    f = dicom.read_file(_write(tmp_path / "g.dcm", _jpeg_file(_one(_good()))))
    assert f.encoding == "jpeg-lossless" and f.jpeg.precision == 16 and f.frame[f.jpeg.offset:f.jpeg.offset + 4].tobytes() == b"\x12\x34\xff\xd9"
    f = dicom.read_file(_write(tmp_path / "p.dcm", _jpeg_file(_one(_good()), syntax=P14)))
    assert f.encoding == "jpeg-lossless" and f.transfer_syntax == P14


def test_defined_length_pixel_data_and_the_other_jpeg_syntaxes_stay_refused(tmp_path):
    for syntax in (SV1, P14):
        path = _write(tmp_path / "d.dcm", D.part10(D.image_elements(), D.slice_bytes(3, 4, "i2")[1], syntax=syntax))
        with pytest.raises(ConfigurationError, match="JPEG lossless.*compressed and needs encapsulated PixelData of undefined length") as err:
            dicom.read_file(path)
        assert path in str(err.value) and syntax in str(err.value)
    for syntax in ("1.2.840.10008.1.2.4.50", "1.2.840.10008.1.2.4.80", "1.2.840.10008.1.2.4.90"):
        path = _write(tmp_path / "o.dcm", _jpeg_file(_one(_good()), syntax=syntax))
        with pytest.raises(ConfigurationError, match="compressed.*only JPEG Lossless") as err:
            dicom.read_file(path)
        assert path in str(err.value) and syntax in str(err.value) and "JPEG / JPEG-LS" not in str(err.value)


# ---- mmnn_jpegll_decode refuses bad arguments before any launch (no GPU: the pointers are fake and never dereferenced) -----------------
@pytest.fixture(scope="module")
def lib():
    return H.built_lib()


_BAD_CALLS = H.bad_calls("frames", too_deep=32)


@pytest.mark.parametrize("name", sorted(_BAD_CALLS))
def test_jpegll_decode_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    H.assert_refused(lib, "mmnn_jpegll_decode", _lib.JpegllDesc, *_BAD_CALLS[name])


def test_jpegll_decode_refuses_a_null_descriptor(lib):
    assert lib.mmnn_jpegll_decode(None, PAY, H.TAB, PIX, STA, WS, None) == 1


def test_jpegll_workspace_bytes_is_monotone_and_refuses_bad_extents(lib):
    from mmnn_sts_amd import _lib
    from mmnn_sts_amd.data import ingest
    size = lambda x, y, z, bits: _lib.count("mmnn_jpegll_workspace_bytes", x, y, z, bits)
    assert _lib.JPEGLL_CHUNK >= 256 and _lib.JPEGLL_CHUNK % 16 == 0 and ingest.JPEGLL_FRAME.itemsize == _lib.JPEGLL_FRAME_BYTES == R.RECORD.itemsize
    assert ingest.JPEGLL_FRAME == R.RECORD
    for bits in (8, 16):
        sizes = [size(*e, bits) for e in ((1, 1, 1), (5, 3, 2), (64, 64, 3), (512, 512, 48), (512, 512, 96), (1024, 512, 96))]
        assert sizes == sorted(sizes) and sizes[0] > 0
    assert size(512, 512, 48, 8) >= 512 * 512 * 48 * 2                                               # the differences are 16-bit words at either width
    for bad in ((0, 4, 4, 16), (4, -1, 4, 16), (4, 4, 0, 8), (2048, 2048, 512, 8), (4, 4, 4, 12), (4, 4, 4, 32), (4, 4, 4, 0)):
        assert lib.mmnn_jpegll_workspace_bytes(*bad) < 0
        with pytest.raises(ValueError, match="jpegll_workspace_bytes"):
            size(*bad)


# ---- the positional core on the host, under the sanitizers -----------------------------------------------------------------------------
def host_check_cases():
    """[(name, x, y, z, bits_allocated, payload, records)]: every stream the GPU test gives the kernel -- the encoder's, the hand-built,
    the malformed at both widths, and records that lie about where the data is."""
    from mmnn_sts_amd import _lib
    cases = []
    for name, (vol, bits_stored) in R.volumes().items():
        for table in ("default", "frame"):
            payload, records = R.pack_fragments(_fragments(vol, bits_stored, table))
            cases.append((f"{name}_{table}", *vol.shape, vol.dtype.itemsize * 8, payload, records))
    for name, (x, y, bits, streams) in R.hand_streams(_lib.JPEGLL_CHUNK).items():
        payload, records = R.pack_payload(streams)
        cases.append((name, x, y, len(streams), bits, payload, records))
    for name in R.malformed_streams():
        for bits in (8, 16):
            streams, x, y, _ = R.malformed_frames(name, bits)
            payload, records = R.pack_payload(streams)
            cases.append((f"malformed_{name}_{bits}", x, y, 3, bits, payload, records))
    for name, (streams, patch) in R.lying_records().items():
        payload, records = R.pack_payload(streams)
        patch(records, payload)
        cases.append((f"lie_{name}", 8, 6, 3, 8, payload, records))
    return cases


def test_positional_core_on_the_host_under_sanitizers(tmp_path):
    cases = host_check_cases()
    results = H.run_host_check(tmp_path, "jpegll_core_check", [c[1:] for c in cases], R.RECORD)
    for (name, x, y, z, bits, payload, records), got in zip(cases, results):
        _, status = H.assert_equals_restatement(name, got, R.decode_ref(payload, records, x, y, bits), who="host check")
        if name.startswith(("malformed_", "lie_")):
            assert status.tolist() == [0, 1, 0], name
        else:
            assert not status.any(), name
