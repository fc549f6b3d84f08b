"""The JPEG Lossless path on the device.  `mmnn_jpegll_decode` against the restatement of its contract (tests/_dicom_jpegll_ref.py), bit for
bit on pixels and status, with every buffer inside a patterned guard buffer; a synth_nifti tree against its uncompressed, RLE and JPEG
Lossless DICOM twins through `IngestCollate`, bit for bit (derived, not measured: the decode is exact integer work and everything behind
it is the code the uncompressed twin runs); and a series with a truncated stream, refused with its file named.

Every stream here, the malformed ones first of all, passes the stand-alone host check of the positional core under the sanitizers
(tests/test_dicom_jpegll_cpu.py::test_positional_core_on_the_host_under_sanitizers takes the same cases from `host_check_cases`)."""
import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import cache as C
from mmnn_sts_amd.data import dicom, ingest, synth_dicom, synth_nifti
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _dicom_jpegll_ref as R
from tests import _dicom_stream_harness as H
from tests._dicom_stream_harness import DEV, dataset as _dataset

pytestmark = pytest.mark.gpu


def _decode(payload, records, x, y, bits):
    """The kernel's (pixels (z, y, x), status (z,)) through `H.guarded_call`."""
    rec = np.ascontiguousarray(records, dtype=R.RECORD).view(np.uint8).reshape(-1)
    return H.guarded_call("mmnn_jpegll_decode", _lib.JpegllDesc, "frames", rec, payload, x, y, len(records), bits)


def _assert_equals_restatement(name, payload, records, x, y, bits):
    return H.assert_equals_restatement(name, _decode(payload, records, x, y, bits), R.decode_ref(payload, records, x, y, bits))


@pytest.mark.parametrize("table", ["default", "frame"])
@pytest.mark.parametrize("name", sorted(R.volumes()))
def test_encoded_volumes_decode_to_the_uncompressed_bytes(name, table):
    vol, bits_stored = R.volumes()[name]
    x, y, z = vol.shape
    fragments = [synth_dicom.jpeg_lossless_fragment(vol[:, :, k].T, bits_stored, table) for k in range(z)]
    payload, records = R.pack_fragments(fragments)
    pixels, status = _assert_equals_restatement(name, payload, records, x, y, vol.dtype.itemsize * 8)
    assert not status.any() and pixels.tobytes() == vol.astype(vol.dtype.newbyteorder("<")).tobytes(order="F")
    if name == "64x64x2_i2_noise" and table == "default":          # about 16 KB a frame and 2 700 stuffed pairs: many chunks, heavy stuffing
        assert all(int(r["length"]) > 12 * _lib.JPEGLL_CHUNK for r in records) and fragments[0].count(b"\xff\x00") > 2000


@pytest.mark.parametrize("name", sorted(R.hand_streams(_lib.JPEGLL_CHUNK)))
def test_hand_built_streams(name):
    x, y, bits, streams = R.hand_streams(_lib.JPEGLL_CHUNK)[name]
    payload, records = R.pack_payload(streams)
    _, status = _assert_equals_restatement(name, payload, records, x, y, bits)
    assert not status.any()
    if name in ("one_bit_symbols", "31_bit_symbols") or name.startswith("straddles"):
        assert int(records[0]["length"]) > _lib.JPEGLL_CHUNK


def test_two_calls_give_identical_bytes():
    x, y, bits, streams = R.hand_streams(_lib.JPEGLL_CHUNK)["31_bit_symbols"]
    payload, records = R.pack_payload(streams)
    a, b = (_decode(payload, records, x, y, bits) for _ in range(2))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _alone(streams, k, x, y, bits):
    payload, records = R.pack_payload([streams[k]])
    pixels, status = R.decode_ref(payload, records, x, y, bits)
    assert not status.any()
    return pixels[0]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", sorted(R.malformed_streams()))
def test_malformed_stream_fails_its_frame_alone(name, bits):
    streams, x, y, _ = R.malformed_frames(name, bits)
    payload, records = R.pack_payload(streams)
    pixels, status = _assert_equals_restatement(name, payload, records, x, y, bits)
    assert status.tolist() == [0, 1, 0]
    for k in (0, 2):                            # the sound frames, against their own streams alone
        assert np.array_equal(pixels[k], _alone(streams, k, x, y, bits))


@pytest.mark.parametrize("name", sorted(R.lying_records()))
def test_records_that_lie_are_clamped(name):
    streams, patch = R.lying_records()[name]
    payload, records = R.pack_payload(streams)
    patch(records, payload)
    pixels, status = _assert_equals_restatement(name, payload, records, 8, 6, 8)
    assert status.tolist() == [0, 1, 0]
    for k in (0, 2):
        assert np.array_equal(pixels[k], _alone(streams, k, 8, 6, 8))


# ---- a NIfTI tree, its uncompressed, RLE and JPEG Lossless twins through the collate ----------------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpegll_twins")
    n = synth_nifti.write_tree(root / "nifti", n_patients=2, seed=21)
    d = synth_dicom.from_nifti_tree(root / "nifti", root / "native", seed=21)
    r = synth_dicom.from_nifti_tree(root / "nifti", root / "rle", seed=21, transfer_syntax="rle")
    j = synth_dicom.from_nifti_tree(root / "nifti", root / "jpeg", seed=21, transfer_syntax="jpeg-lossless")
    return n, d, r, j


def test_four_twins_give_the_same_batch(trees):
    sets = [_dataset(t) for t in trees]
    assert [s.layout for s in sets] == ["nifti", "dicom", "dicom", "dicom"] and sets[0].uids == sets[1].uids == sets[2].uids == sets[3].uids
    for scan, mask in sets[3][0][0].volumes:    # the scan AND the mask are JPEG Lossless series
        assert scan.encoding == mask.encoding == "jpeg-lossless" and mask.bits_allocated == 8 and scan.bits_allocated == 16
        assert sum(f.size for f in scan.frames) < scan.shape[0] * scan.shape[1] * scan.shape[2] * 2
    assert all(scan.encoding == "rle" for scan, _ in sets[2][0][0].volumes)
    results = []
    for ds, threshold in zip(sets, (0.5, None, None, None)):      # a DICOM pair is resampled and binarised at 128 (tests/test_dicom_gpu.py)
        collate = ingest.IngestCollate(DEV, mask_threshold=threshold, size=64)
        x, ev, du = collate([ds[0], ds[1]])
        torch.cuda.synchronize()
        results.append((x, collate.pending[-1][1]))
    (x_n, e_n), (x_d, e_d), (x_r, e_r), (x_j, e_j) = results
    assert x_n.shape == (2, 2, 64, 64, 64) and float(x_n.abs().max()) > 0.0 and int(e_n.min()) > 0
    assert torch.equal(e_n, e_d) and torch.equal(e_d, e_r) and torch.equal(e_r, e_j)
    assert torch.equal(x_d, x_j), f"{int((x_d != x_j).sum())} elements differ between the uncompressed and the JPEG Lossless twin"
    assert torch.equal(x_r, x_j), f"{int((x_r != x_j).sum())} elements differ between the RLE and the JPEG Lossless twin"
    assert torch.equal(x_n, x_j), f"{int((x_n != x_j).sum())} elements differ between the NIfTI tree and the JPEG Lossless twin"


def test_jpeg_twin_through_the_volume_cache(trees):
    from mmnn_sts_amd.data.ImageDatasets import ImageDatasetByUIDs
    native, jpeg = _dataset(trees[1]), _dataset(trees[3])
    plain = ingest.IngestCollate(DEV, mask_threshold=None)
    want, _, _ = plain([native[0], native[1]])
    want_extents = plain.pending[-1][1]
    cache = C.VolumeCache(DEV, 2, 64, 2)
    collate = ingest.IngestCollate(DEV, mask_threshold=None, cache=cache)
    sub = C.CachedByUIDs(jpeg, jpeg.uids, cache)
    for what in ("filling the cache", "from the cache"):
        got, _, _ = collate([sub[0], sub[1]])
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(collate.pending[-1][1], want_extents), what
    assert isinstance(sub[0][0], C.CachedPatient) and isinstance(ImageDatasetByUIDs(jpeg, jpeg.uids)[0][0], ingest.RawPatient)


def test_a_truncated_stream_is_refused_with_its_file_named_and_the_next_series_ingests(tmp_path):
    vol = np.random.default_rng(9).integers(-300, 300, (20, 12, 4)).astype("i2")
    for sub in ("good", "bad"):
        synth_dicom.write_series(tmp_path / sub, vol, slope=0.5, inter=-3.0, shuffle_names=False, bits_stored=12, transfer_syntax="jpeg-lossless")
    victim = str(tmp_path / "bad" / "0002.dcm")
    data = open(victim, "rb").read()
    head = dicom.read_file(victim, header_only=True)
    # drop the last 40 bytes of the fragment: the item grows shorter, the marker segments stay right, the host finds no fault
    at = data.rindex(b"\xfe\xff\x00\xe0")
    length = int.from_bytes(data[at + 4:at + 8], "little")
    cut = data[:at + 4] + (length - 40).to_bytes(4, "little") + data[at + 8:at + 8 + length - 40] + data[at + 8 + length:]
    with open(victim, "wb") as f:
        f.write(cut)
    series = dicom.read_series(tmp_path / "bad")
    assert series.encoding == "jpeg-lossless" and series.jpeg[2].length == head.jpeg.length - 40 and series.jpeg[2].precision == 16
    with pytest.raises(ConfigurationError, match="the JPEG stream ends, or holds an invalid code, before its 20 x 12 samples are decoded") as err:
        ingest.upload(series, DEV)
    assert victim in str(err.value)
    v = ingest.upload(dicom.read_series(tmp_path / "good"), DEV)
    torch.cuda.synchronize()
    assert v.from_dicom and v.datatype == 4 and (v.slope, v.inter) == (0.5, -3.0)
    assert np.array_equal(np.frombuffer(v.data.cpu().numpy().tobytes(), dtype="<i2").reshape(vol.shape, order="F"), vol)
