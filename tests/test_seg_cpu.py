"""`not gpu` side of the DICOM SEG path: the reader (`mmnn_sts_amd.data.seg`) against files packed here with struct at the published
element layout (tests/_seg_ref.py shares no code with the package), segment selection, the placement of frames against a scan's grid,
the round trip of `synth_dicom.write_seg` through the numpy restatement of the bit order, the datasets' detection of a SEG mask and
`Data: mask_roi`, and the host-side refusals of `mmnn_unpack_frames`."""
import ctypes
import logging
import os
import shutil

import numpy as np
import pytest

from mmnn_sts_amd.data import seg, synth_dicom, synth_nifti
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _resample_ref as G
from tests import _seg_ref as S

ROWS, COLS = 3, 5
SEGMENTS = [(4, "Body"), (9, "GTV 1")]
# (segment number, position): frame order in the file is neither by segment nor by position
FRAMES = [(9, (0.0, 0.0, 4.0)), (4, (0.0, 0.0, 0.0)), (9, (0.0, 0.0, 0.0)), (9, (0.0, 0.0, 6.0))]


def _write(path, data):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def _planes(n=len(FRAMES), rows=ROWS, cols=COLS, seed=3):
    return [(np.random.default_rng([seed, f]).random((rows, cols)) < 0.5).astype(np.uint8) for f in range(n)]


def _file(**kw):
    args = dict(rows=ROWS, columns=COLS, segments=SEGMENTS, frames=FRAMES, pixels=S.pack_frames(_planes()))
    args.update(kw)
    return S.seg_file(**args)


# ---- the reader ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["shared", "frame"])
@pytest.mark.parametrize("undefined", [False, True])
@pytest.mark.parametrize("explicit", [True, False])
def test_reader_walks_sequences_in_both_vr_modes_and_length_forms(tmp_path, explicit, undefined, where):
    pixels = S.pack_frames(_planes())
    path = _write(tmp_path / "s.dcm", _file(explicit=explicit, undefined=undefined, where=where, orientation=(0, 1, 0, -1, 0, 0),
                                            spacing=(0.5, 0.25), thickness=2.5, between=2.0))
    fs = seg.read(path)
    assert fs.names == ["Body", "GTV 1"] and (fs.rows, fs.columns, fs.n_frames) == (ROWS, COLS, 4) and not fs.header_only
    assert fs.segment_of.tolist() == [1, 0, 1, 1]
    assert np.array_equal(fs.positions, [p for _, p in FRAMES]) and np.array_equal(fs.orientations, [(0, 1, 0, -1, 0, 0)] * 4)
    assert np.array_equal(fs.spacings, [(0.5, 0.25)] * 4) and fs.steps.tolist() == [2.0] * 4          # SpacingBetweenSlices over SliceThickness
    assert fs.frame.dtype == np.uint8 and fs.frame.size == (4 * ROWS * COLS + 7) // 8 == 8
    assert bytes(fs.frame) == pixels[:8] and not fs.frame.flags.owndata and not fs.frame.flags.writeable   # a view of the mapped file
    head = seg.read(path, header_only=True)
    assert head.names == fs.names and head.header_only and head.frame is None and np.array_equal(head.positions, fs.positions)
    assert seg.sop_class_of(path) == seg.SEGMENTATION_STORAGE


def test_header_only_stops_in_front_of_pixel_data(tmp_path):
    """A file cut off inside PixelData still gives its frames header-only, and is refused as truncated when read in full."""
    data = _file()
    path = _write(tmp_path / "cut.dcm", data[:-6])
    head = seg.read(path, header_only=True)
    assert head.frame is None and head.n_frames == 4
    with pytest.raises(ConfigurationError, match=r"cut\.dcm: truncated: 2 bytes of PixelData, 8 expected for 4 frames of 3 x 5 bits"):
        seg.read(path)
    # the declared length itself too short for the frames
    short = _write(tmp_path / "short.dcm", _file(pixels=S.pack_frames(_planes())[:6]))
    with pytest.raises(ConfigurationError, match=r"short\.dcm: truncated: 6 bytes of PixelData, 8 expected"):
        seg.read(short)


def test_selection_rules(tmp_path):
    fs = seg.read(_write(tmp_path / "two.dcm", _file()))
    for name in ("GTV 1", "gtv 1", "Gtv 1"):
        one = seg.select(fs, name)
        assert one.names == ["GTV 1"] and one.segment_of.tolist() == [0, -1, 0, 0] and one.frame is fs.frame
    assert seg.select(fs, "BODY").segment_of.tolist() == [-1, 0, -1, -1]
    with pytest.raises(ConfigurationError, match=r"two\.dcm holds 2 segments \('Body', 'GTV 1'\).*mask_roi"):
        seg.select(fs, None)                                                            # several segments and no name
    with pytest.raises(ConfigurationError, match="no segment labelled 'GTV'.*'Body', 'GTV 1'"):
        seg.select(fs, "GTV")                                                           # exact, not a prefix
    single = seg.read(_write(tmp_path / "one.dcm", _file(segments=SEGMENTS[1:], frames=[f for f in FRAMES if f[0] == 9],
                                                          pixels=S.pack_frames(_planes(3)))))
    assert seg.select(single, None).names == ["GTV 1"] and seg.select(seg.select(fs, "gtv 1"), None).names == ["GTV 1"]
    with pytest.raises(ConfigurationError, match="no segment labelled"):
        seg.select(single, "Body")


_REFUSED = {
    "another SOP class": (dict(sop_class="1.2.840.10008.5.1.4.1.1.4"), "is not Segmentation Storage"),
    "fractional": (dict(kind="FRACTIONAL", bits=8, pixels=bytes(60)), "SegmentationType FRACTIONAL.*export as BINARY"),
    "labelmap": (dict(kind="LABELMAP", bits=8, pixels=bytes(60)), "SegmentationType LABELMAP.*export as BINARY"),
    "eight bits": (dict(bits=8, pixels=bytes(60)), "BitsAllocated 8.*export as BINARY"),
    "big endian": (dict(syntax="1.2.840.10008.1.2.2"), "big endian"),
    "deflated": (dict(syntax="1.2.840.10008.1.2.1.99"), "deflated"),
    "jpeg": (dict(syntax="1.2.840.10008.1.2.4.70"), "encapsulated"),
    "rle": (dict(syntax="1.2.840.10008.1.2.5"), "RLE.*decompress the file first"),
    "frame count": (dict(declared_frames=5), "NumberOfFrames 5 and 4 items"),
    "no position": (dict(frames=FRAMES[:2] + [(9, None)] + FRAMES[3:]), "frame 2 has no PlanePositionSequence"),
    "no segment number": (dict(frames=FRAMES[:1] + [(None, (0.0, 0.0, 0.0))] + FRAMES[2:]), "frame 1 has no SegmentIdentificationSequence"),
    "no orientation": (dict(where=None), "no PlaneOrientationSequence / ImageOrientationPatient"),
    "unknown segment": (dict(frames=FRAMES[:3] + [(5, (0.0, 0.0, 6.0))]), "frame 3 refers to SegmentNumber 5"),
}


@pytest.mark.parametrize("name", sorted(_REFUSED))
def test_files_outside_the_path_are_refused_with_the_path_and_a_reason(tmp_path, name):
    fields, reason = _REFUSED[name]
    path = _write(tmp_path / "bad.dcm", _file(**fields))
    with pytest.raises(ConfigurationError, match=r"bad\.dcm: .*" + reason):
        seg.read(path)


def test_a_file_without_the_magic_is_no_dicom(tmp_path):
    from mmnn_sts_amd.data.dicom import NotDicomError
    with pytest.raises(NotDicomError):
        seg.read(_write(tmp_path / "text.dcm", b"no magic here " * 20))
    with pytest.raises(NotDicomError):
        seg.sop_class_of(tmp_path / "text.dcm")


# ---- placement -------------------------------------------------------------------------------------------------------------------------
def _placed(tmp_path, positions, rows=6, cols=6, **kw):
    frames = [(9, p) for p in positions]
    path = _write(tmp_path / "p.dcm", S.seg_file(rows, cols, [(9, "GTV")], frames, S.pack_frames(_planes(len(frames), rows, cols)), **kw))
    return seg.read(path, header_only=True)


def test_frames_on_the_scans_grid_give_refs_and_slice_first(tmp_path):
    positions = [(0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 0.0, 4.0), (0.0, 0.0, 6.0)]         # slices 2, 0, 2, 3: two frames on slice 2
    fs = _placed(tmp_path, positions)
    place = seg.to_scan(fs, (6, 6, 4), S.LPS_AFFINE)
    assert place.on_scan and place.one == 1 and place.shape == (6, 6, 4) and np.array_equal(place.affine, S.LPS_AFFINE) and place.dropped == 0
    assert place.refs.dtype == np.int32 and place.slice_first.dtype == np.int32
    assert place.refs.tolist() == [1, 0, 2, 3] and place.slice_first.tolist() == [0, 1, 1, 3, 4]
    assert S.on_scan_ref(positions, (1, 0, 0, 0, 1, 0), (1.0, 1.0), (6, 6, 4), S.LPS_AFFINE) == [2, 0, 2, 3]
    want = S.arrays([2, 0, 2, 3], [0, 1, 2, 3], 4)
    assert np.array_equal(place.refs, want[0]) and np.array_equal(place.slice_first, want[1])
    # 4e-4 voxel off is still the scan's grid; other extents are not
    assert seg.to_scan(_placed(tmp_path, [(4e-4, 0.0, 2.0)]), (6, 6, 4), S.LPS_AFFINE).on_scan
    assert not seg.to_scan(fs, (6, 5, 4), S.LPS_AFFINE).on_scan


def test_frames_outside_the_scan_are_dropped_counted_and_reported_once(tmp_path, caplog):
    fs = _placed(tmp_path, [(0.0, 0.0, 2.0), (0.0, 0.0, 8.0), (0.0, 0.0, -2.0)])
    with caplog.at_level(logging.WARNING, logger="mmnn_sts_amd.data.seg"):
        first, second = seg.to_scan(fs, (6, 6, 4), S.LPS_AFFINE), seg.to_scan(fs, (6, 6, 4), S.LPS_AFFINE)
    assert first.dropped == second.dropped == 2 and first.refs.tolist() == [0] and first.slice_first.tolist() == [0, 0, 1, 1, 1]
    warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "p.dcm" in warnings[0] and "2 frame(s)" in warnings[0] and "outside the scan" in warnings[0]
    with pytest.raises(ConfigurationError, match=r"p\.dcm: segment 'GTV' leaves nothing on the scan's 4 slices"):
        seg.to_scan(_placed(tmp_path, [(0.0, 0.0, 8.0)]), (6, 6, 4), S.LPS_AFFINE)
    with pytest.raises(ConfigurationError, match="no geometry"):
        seg.to_scan(fs, (6, 6, 4), None)


def test_frames_half_a_voxel_off_form_a_grid_of_their_own_with_two_empty_end_slices(tmp_path):
    positions = [(0.5, 0.0, 6.0), (0.5, 0.0, 2.0)]                                            # half a voxel along x; two steps apart
    fs = _placed(tmp_path, positions, thickness=2.0)
    place = seg.to_scan(fs, (6, 6, 4), S.LPS_AFFINE)
    assert not place.on_scan and place.one == 255 and place.from_dicom and place.shape == (6, 6, 5)
    # first occupied slice is 1, the last one 3; 0 and 4 are empty; the affine's origin is one step below the first frame
    assert place.refs.tolist() == [1, 0] and place.slice_first.tolist() == [0, 0, 1, 1, 2, 2]
    assert np.array_equal(place.affine, [[-1.0, 0.0, 0.0, -0.5], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    shape, affine, slices = S.own_grid_ref(positions, (1, 0, 0, 0, 1, 0), (1.0, 1.0), 2.0, 6, 6)
    assert shape == place.shape and slices == [3, 1] and np.abs(affine - place.affine).max() <= 1e-12
    # the step: SpacingBetweenSlices, else SliceThickness, else the smallest positive gap
    assert seg.to_scan(_placed(tmp_path, positions, thickness=1.0, between=2.0), (6, 6, 4), S.LPS_AFFINE).shape == (6, 6, 5)
    assert seg.to_scan(_placed(tmp_path, positions, thickness=1.0), (6, 6, 4), S.LPS_AFFINE).shape == (6, 6, 7)
    assert seg.to_scan(_placed(tmp_path, positions + [(0.5, 0.0, 4.0)], thickness=None), (6, 6, 4), S.LPS_AFFINE).shape == (6, 6, 5)
    # an oblique stack with anisotropic pixels against the restatement
    A = G.affine((("z", 0.35), ("x", -0.5)), (0.7, 0.9, 3.3), (-41.3, 22.7, -13.9))
    orientation, spacing, first, step = synth_dicom.lps_geometry(A)
    positions = [first + k * step for k in (5, 2, 3)]
    fs = _placed(tmp_path, positions, rows=4, cols=7, orientation=orientation, spacing=spacing, thickness=3.3)
    place = seg.to_scan(fs, (9, 9, 9), np.eye(4))
    shape, affine, slices = S.own_grid_ref(positions, orientation, spacing, 3.3, 4, 7)
    assert place.shape == shape == (7, 4, 6) and np.abs(affine - place.affine).max() <= 1e-9
    assert place.refs.tolist() == [1, 2, 0] and place.slice_first.tolist() == [0, 0, 1, 2, 2, 3, 3]
    assert np.abs(place.affine @ [0, 0, 1, 1] - A @ [0, 0, 2, 1]).max() <= 1e-9                # slice 1 is the lowest frame, the mask's slice 2


def test_frames_that_form_no_regular_stack_are_refused_with_the_frame_named(tmp_path):
    with pytest.raises(ConfigurationError, match=r"p\.dcm: frame 1 of segment 'GTV' lies 1\.5 steps of 2 mm"):
        seg.to_scan(_placed(tmp_path, [(0.5, 0.0, 2.0), (0.5, 0.0, 5.0)], thickness=2.0), (6, 6, 4), S.LPS_AFFINE)
    with pytest.raises(ConfigurationError, match=r"p\.dcm: frame 1 of segment 'GTV' is shifted 0\.25 voxel in its plane"):
        seg.to_scan(_placed(tmp_path, [(0.5, 0.0, 2.0), (0.75, 0.0, 4.0)], thickness=2.0), (6, 6, 4), S.LPS_AFFINE)
    data = S.seg_file(6, 6, [(9, "GTV")], [(9, (0.5, 0.0, 2.0)), (9, (0.5, 0.0, 4.0))], S.pack_frames(_planes(2, 6, 6)), where="frame")
    tilted = data.replace(b"1.0\\0.0\\0.0\\0.0\\1.0\\0.0", b"1.0\\0.0\\0.0\\0.0\\0.8\\0.6", 1)
    assert tilted != data
    with pytest.raises(ConfigurationError, match="frames 0 and 1 of segment 'GTV' differ in ImageOrientationPatient"):
        seg.to_scan(seg.read(_write(tmp_path / "t.dcm", tilted), header_only=True), (6, 6, 4), S.LPS_AFFINE)


# ---- the writer's round trip on an oblique geometry --------------------------------------------------------------------------------------
OBLIQUE = G.affine((("z", 0.35), ("x", -0.5), ("y", 0.8)), (0.7, 0.9, 3.3), (-41.3, 22.7, -13.9))


@pytest.mark.parametrize("explicit,undefined,per_frame", [(True, False, False), (False, True, True)])
def test_write_seg_comes_back_as_the_mask(tmp_path, explicit, undefined, per_frame):
    rng = np.random.default_rng(12)
    mask = (rng.random((37, 29, 6)) < 0.45).astype(np.uint8)
    mask[:, :, 3] = 0                                                                    # a slice without a frame
    other = (rng.random((37, 29, 6)) < 0.2).astype(np.uint8)
    path = synth_dicom.write_seg(tmp_path / "m" / "seg.dcm", mask, OBLIQUE, "GTV", ("Body", ("Node", other)), explicit, undefined,
                                 per_frame_orientation=per_frame, seed=5)
    fs = seg.read(path)
    assert fs.names == ["Body", "GTV", "Node"] and fs.n_frames == 1 + 5 + 6 and (37 * 29) % 8 != 0
    one = seg.select(fs, "gtv")
    place = seg.to_scan(one, mask.shape, OBLIQUE)
    assert place.on_scan and place.dropped == 0 and place.slice_first.tolist() == [0, 1, 2, 3, 3, 4, 5]
    assert place.refs.tolist() != sorted(place.refs.tolist())                            # the frames are not in slice order in the file
    chosen = np.flatnonzero(one.segment_of == 0)
    assert not np.array_equal(chosen, np.arange(chosen[0], chosen[0] + 5))               # ... and the other segments' lie between them
    ks = S.on_scan_ref(fs.positions[place.refs], fs.orientations[0], fs.spacings[0], mask.shape, OBLIQUE)
    assert ks == [0, 1, 2, 4, 5]
    assert np.array_equal(S.unpack_ref(fs.frame, fs.n_frames, place.refs, place.slice_first, mask.shape), mask)
    node = seg.to_scan(seg.select(fs, "Node"), mask.shape, OBLIQUE)
    assert np.array_equal(S.unpack_ref(fs.frame, fs.n_frames, node.refs, node.slice_first, mask.shape, 255), other * 255)
    body = seg.to_scan(seg.select(fs, "body"), mask.shape, OBLIQUE)
    decoy = S.unpack_ref(fs.frame, fs.n_frames, body.refs, body.slice_first, mask.shape)
    assert decoy[:, :, 0].all() and not decoy[:, :, 1:].any()
    # the value has even length, and the pad bits behind the last frame are not all zero for every seed (garbage, not padding)
    pads = set()
    for seed in range(8):
        p = synth_dicom.write_seg(tmp_path / "pad" / f"{seed}.dcm", mask, OBLIQUE, seed=seed)
        f = seg.read(p)
        pad = -(f.n_frames * 37 * 29) % 8
        assert os.path.getsize(p) % 2 == 0 and f.n_frames == 5 and pad == 3
        pads.add(int(f.frame[-1]) >> (8 - pad))
    assert len(pads) > 1
    # on another scan grid the same file forms a stack of its own: five occupied positions over six steps, plus the two end slices
    own = seg.to_scan(one, (40, 30, 6), np.eye(4))
    assert not own.on_scan and own.shape == (37, 29, 8) and own.slice_first.tolist() == [0, 0, 1, 2, 3, 3, 4, 5, 5]
    assert np.abs(own.affine @ [0, 0, 1, 1] - OBLIQUE @ [0, 0, 0, 1]).max() <= 1e-9 and np.abs(own.affine[:3, :3] - OBLIQUE[:3, :3]).max() <= 1e-9


# ---- datasets ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("seg")
    synth_nifti.write_tree(root / "nifti", n_patients=3, seed=11, extent=((8, 12), (8, 12), (4, 6)))
    return synth_dicom.from_nifti_tree(root / "nifti", root / "dicom", mask_format="seg", extra_rois=("Body",))


@pytest.fixture(scope="module")
def own_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("segown")
    synth_nifti.write_tree(root / "nifti", n_patients=3, seed=11, extent=((8, 12), (8, 12), (4, 6)), mask_grid="own")
    return synth_dicom.from_nifti_tree(root / "nifti", root / "dicom", mask_format="seg")


def _dataset(tree, **kw):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"], **kw)


def test_a_tree_with_seg_masks_is_detected_and_constructs(tree):
    from mmnn_sts_amd.data import dicom, ingest
    ds = _dataset(tree, mask_roi="gtv")
    assert ds.layout == "dicom" and len(ds) == 3 and ds.other_grid == []
    raw = ds[0][0]
    assert len(raw.volumes) == 2
    for scan, mask in raw.volumes:
        assert isinstance(scan, dicom.DicomSeries) and isinstance(mask, seg.FrameSet)
        assert mask.names == ["GTV"] and mask.frame is not None and os.path.basename(mask.path) == "seg.dcm"
        assert (mask.columns, mask.rows) == scan.shape[:2] and ingest.mask_index_map(scan, mask) is None


def test_seg_masks_on_their_own_grids_are_counted_and_refused_by_never(own_tree, caplog):
    from mmnn_sts_amd.data import ingest
    with caplog.at_level(logging.INFO, logger="mmnn_sts_amd.data.ImageDatasets"):
        ds = _dataset(own_tree)
    assert len(ds.other_grid) == 3 and any("3 of 3 patients" in r.getMessage() and "another grid" in r.getMessage() for r in caplog.records)
    scan, mask = ds[0][0].volumes[0]
    place = seg.to_scan(mask, scan.shape, scan.affine)
    assert not place.on_scan and place.shape[:2] == (mask.columns, mask.rows) != scan.shape[:2]
    t = ingest.mask_index_map(scan, mask)
    assert t.shape == (3, 4) and np.abs(t - G.index_map(scan.affine, place.affine)).max() <= 1e-9
    with pytest.raises(ConfigurationError, match=r"scan extent \(\d+, \d+, \d+\), SEG extent \(\d+, \d+, \d+\).*mask_resample is 'never'"):
        _dataset(own_tree, mask_resample="never")
    with pytest.raises(ConfigurationError, match=r"scan extent .*SEG extent .*mask_resample is 'never'"):
        ingest.mask_index_map(scan, mask, "never")


def test_a_wrong_mask_roi_fails_at_construction_with_the_labels(tree):
    with pytest.raises(ConfigurationError, match="no segment labelled 'tumour'.*'Body', 'GTV'"):
        _dataset(tree, mask_roi="tumour")
    with pytest.raises(ConfigurationError, match="2 segments \\('Body', 'GTV'\\).*mask_roi"):
        _dataset(tree)


def test_mask_directories_that_mix_are_refused(tree, tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import rtstruct_in, seg_in
    patient = os.path.join(tree["image_loc"], "t1", sorted(os.listdir(os.path.join(tree["image_loc"], "t1")))[0])
    sg = os.path.join(patient, "mask", "seg.dcm")
    assert seg_in(os.path.join(patient, "mask")) == sg and seg_in(os.path.join(patient, "image")) is None
    two = tmp_path / "two" / "mask"
    os.makedirs(two)
    shutil.copyfile(sg, two / "a.dcm")
    shutil.copyfile(sg, two / "b.dcm")
    with pytest.raises(ConfigurationError, match=r"2 DICOM SEG files \(a\.dcm, b\.dcm\)"):
        seg_in(two)
    mixed = tmp_path / "mixed" / "mask"
    os.makedirs(mixed)
    shutil.copyfile(sg, mixed / "seg.dcm")
    series = os.path.join(patient, "image", "series_1")
    shutil.copyfile(os.path.join(series, sorted(os.listdir(series))[0]), mixed / "slice.dcm")
    with pytest.raises(ConfigurationError, match=r"a DICOM SEG file \(seg\.dcm\) beside 1 DICOM image file"):
        seg_in(mixed)
    both = tmp_path / "both" / "mask"
    os.makedirs(both)
    shutil.copyfile(sg, both / "seg.dcm")
    synth_dicom.write_rtstruct(both / "rs.dcm", np.ones((4, 4, 2), dtype=np.uint8), np.eye(4))
    with pytest.raises(ConfigurationError, match=r"a DICOM SEG file \(seg\.dcm\) beside an RTSTRUCT file \(rs\.dcm\)"):
        seg_in(both)
    sub = tmp_path / "sub" / "mask" / "SEG_1"                                            # its single sub-directory
    os.makedirs(sub)
    shutil.copyfile(sg, sub / "seg.dcm")
    assert seg_in(tmp_path / "sub" / "mask") == str(sub / "seg.dcm")
    assert rtstruct_in(os.path.join(patient, "image")) is None


def test_one_scan_of_a_mask_directory_classifies_it_and_refuses_mixtures(tmp_path, monkeypatch):
    """The datasets look at a mask/ directory once: every file in it is classified by one `seg.sop_class_of` call per dataset, whatever
    it turns out to hold, and the refusals that used to hang on the order of two scans come from that one."""
    from mmnn_sts_amd.data import dicom, rtstruct
    from mmnn_sts_amd.data.ImageDatasets import ImageSurvivalDataset
    synth_nifti.write_tree(tmp_path / "nifti", n_patients=1, seed=4, extent=((6, 6), (6, 6), (4, 4)), modalities=("t1",))
    trees = {f: synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / f, mask_format=f) for f in ("series", "rtstruct", "seg")}
    calls = {}

    def counted(path, inner=seg.sop_class_of):
        calls[os.path.realpath(str(path))] = calls.get(os.path.realpath(str(path)), 0) + 1
        return inner(path)

    monkeypatch.setattr(seg, "sop_class_of", counted)

    def construct(tree):
        calls.clear()
        try:
            return ImageSurvivalDataset(os.path.join(tree["image_loc"], "t1"), tree["data_loc"], tree["key_loc"])
        finally:
            patient = os.path.join(tree["image_loc"], "t1", os.listdir(os.path.join(tree["image_loc"], "t1"))[0])
            inside = [os.path.realpath(os.path.join(d, f)) for d, _, files in os.walk(os.path.join(patient, "mask")) for f in files]
            assert calls == {p: 1 for p in inside}, calls          # each file of mask/ once, no file of image/ at all

    for name, kind in (("series", dicom.DicomSeries), ("rtstruct", rtstruct.ContourSet), ("seg", seg.FrameSet)):
        ds = construct(trees[name])
        scan, mask = ds[0][0].volumes[0]
        assert isinstance(scan, dicom.DicomSeries) and type(mask) is kind
        assert max(calls.values()) == 1                           # loading a patient does not look again

    def mask_directory(tree):
        t1 = os.path.join(tree["image_loc"], "t1")
        return os.path.join(t1, os.listdir(t1)[0], "mask")

    rs = os.path.join(mask_directory(trees["rtstruct"]), "rtstruct.dcm")
    shutil.copyfile(rs, os.path.join(mask_directory(trees["seg"]), "rtstruct.dcm"))
    with pytest.raises(ConfigurationError, match=r"a DICOM SEG file \(seg\.dcm\) beside an RTSTRUCT file \(rtstruct\.dcm\)"):
        construct(trees["seg"])
    series = os.path.join(mask_directory(trees["series"]), "series_1")
    shutil.copyfile(os.path.join(series, sorted(os.listdir(series))[0]), os.path.join(mask_directory(trees["rtstruct"]), "slice.dcm"))
    with pytest.raises(ConfigurationError, match=r"an RTSTRUCT file \(rtstruct\.dcm\) beside 1 DICOM image file\(s\)"):
        construct(trees["rtstruct"])


def test_a_seg_mask_beside_a_nifti_scan_is_refused(tree):
    from mmnn_sts_amd.data import ingest, nifti
    ds = _dataset(tree, mask_roi="gtv")
    frames = ds[0][0].volumes[0][1]
    scan = nifti.NiftiImage(np.zeros((8, 8, 4), dtype=np.int16), 4, 1.0, 0.0, "scan.nii", np.eye(4))
    with pytest.raises(ConfigurationError, match="DICOM SEG mask beside a NIfTI scan"):
        ingest.mask_index_map(scan, frames)
    with pytest.raises(ConfigurationError, match="DICOM SEG mask .*beside a NIfTI scan"):
        ingest.stage_frames(frames, scan, "cpu")


def test_parser_hands_mask_roi_to_the_datasets(tree):
    import argparse
    from mmnn_sts_amd.parser.parser import Parser
    p = Parser()
    p.parseConfig()
    p.config["Data"] = dict({k: tree[k] for k in ("image_loc", "key_loc", "data_loc")}, t1_path="t1", t2_path="t2", mask_roi="GTV")
    args = argparse.Namespace(classification=False, survival=True, images=True, preop=False, postop=False)
    ds = p.getDatasets(args, p.getImagePath())
    assert ds.mask_roi == "GTV" and p.image_layout == "dicom"
    p.config["Data"]["mask_roi"] = "nothing"
    with pytest.raises(ConfigurationError, match="no segment labelled 'nothing'"):
        p.getDatasets(args, p.getImagePath())


# ---- mmnn_unpack_frames refuses bad arguments before any launch (no GPU: the pointers are fake and never dereferenced) --------------------
@pytest.fixture(scope="module")
def lib():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


B, R, F, O = 0x7F0000100001, 0x7F0000200000, 0x7F0000300000, 0x7F0000900003
_GOOD = dict(x=8, y=4, z=2, n_frames=3, n_refs=2, one=1)
_BAD_CALLS = {
    "zero extent": (dict(y=0), B, R, F, O, "non-positive extent"), "negative extent": (dict(z=-3), B, R, F, O, "non-positive extent"),
    "2^31 voxels": (dict(x=2048, y=2048, z=512), B, R, F, O, "2\\^31 voxels"),
    "negative n_frames": (dict(n_frames=-1), B, R, F, O, "n_frames"), "negative n_refs": (dict(n_refs=-1), B, R, F, O, "n_refs"),
    "one is zero": (dict(one=0), B, R, F, O, "one = 0 outside 1..255"), "one is 256": (dict(one=256), B, R, F, O, "one = 256 outside 1..255"),
    "null bits": ({}, 0, R, F, O, "null"), "null refs": ({}, B, 0, F, O, "null"), "null slice_first": ({}, B, R, 0, O, "null"),
    "null out": ({}, B, R, F, 0, "null"), "null slice_first without refs": (dict(n_refs=0), 0, 0, 0, O, "null"),
    "refs misaligned": ({}, B, R + 2, F, O, "not aligned"), "slice_first misaligned": ({}, B, R, F + 1, O, "not aligned"),
    "out inside bits": (dict(x=64, y=64, n_frames=8), B, R, F, B + 100, "overlap"), "bits inside out": ({}, O + 40, R, F, O, "overlap"),
}


@pytest.mark.parametrize("name", sorted(_BAD_CALLS))
def test_unpack_frames_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    fields, bits, refs, slice_first, out, reason = _BAD_CALLS[name]
    desc = _lib.UnpackFramesDesc(**dict(_GOOD, **fields))
    assert lib.mmnn_unpack_frames(ctypes.byref(desc), bits or None, refs or None, slice_first or None, out or None, None) == 1
    with pytest.raises(ValueError, match=reason):
        _lib.check(1, "mmnn_unpack_frames")


def test_unpack_frames_refuses_a_null_descriptor(lib):
    from mmnn_sts_amd import _lib
    assert lib.mmnn_unpack_frames(None, B, R, F, O, None) == 1
    with pytest.raises(ValueError, match="null descriptor"):
        _lib.check(1, "mmnn_unpack_frames")
