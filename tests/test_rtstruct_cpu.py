"""`not gpu` side of the RTSTRUCT path: the reader (`mmnn_sts_amd.data.rtstruct`) against files packed here with struct at the published
element layout (tests/_rtstruct_ref.py shares no code with the package), ROI selection, the placement of contours on a scan's grid, the
run-rectangle round trip of `synth_dicom.write_rtstruct` through the numpy restatement of the fill rule, the datasets' detection of an
RTSTRUCT mask and `Data: mask_roi`, and the host-side refusals of `mmnn_rasterize_contours`."""
import ctypes
import logging
import os

import numpy as np
import pytest

from mmnn_sts_amd.data import rtstruct, synth_dicom, synth_nifti
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _dicom_ref as D
from tests import _resample_ref as G
from tests import _rtstruct_ref as C


def _write(path, data):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def _two_rois():
    gtv = [("CLOSED_PLANAR", C.square(2), None), ("CLOSED_PLANAR", C.square(0, 0.5, 2.25), None), ("CLOSED_PLANAR", C.square(2, 2.0, 3.0), None)]
    body = [("CLOSED_PLANAR", C.square(1, 0.0, 5.0), None)]
    return [("Body", body), ("GTV 1", gtv)]


# ---- the reader ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("undefined", [False, True])
@pytest.mark.parametrize("explicit", [True, False])
def test_reader_walks_sequences_in_both_vr_modes_and_length_forms(tmp_path, explicit, undefined):
    path = _write(tmp_path / "s.dcm", C.rtstruct_file(_two_rois(), explicit, undefined))
    cs = rtstruct.read(path)
    assert cs.names == ["Body", "GTV 1"] and cs.frames == ["1.2.3.9", "1.2.3.9"] and not cs.header_only
    assert [len(c) for c in cs.contours] == [1, 3] and cs.dropped == [{}, {}]
    assert np.array_equal(cs.contours[0][0], C.square(1, 0.0, 5.0))                        # joined by ROI number: the file lists GTV first
    for got, want in zip(cs.contours[1], (C.square(2), C.square(0, 0.5, 2.25), C.square(2, 2.0, 3.0))):
        assert got.dtype == np.float64 and got.shape == (4, 3) and np.array_equal(got, want)
    head = rtstruct.read(path, header_only=True)
    assert head.names == cs.names and head.header_only and head.contours == [[], []]


def test_header_only_stops_behind_the_roi_names(tmp_path):
    """A file cut off inside ROIContourSequence still gives its names header-only, and is refused as truncated when read in full."""
    data = C.rtstruct_file(_two_rois())
    path = _write(tmp_path / "cut.dcm", data[:-40])
    assert rtstruct.read(path, header_only=True).names == ["Body", "GTV 1"]
    with pytest.raises(ConfigurationError, match="malformed"):
        rtstruct.read(path)


def test_selection_rules(tmp_path):
    cs = rtstruct.read(_write(tmp_path / "two.dcm", C.rtstruct_file(_two_rois())))
    for name in ("GTV 1", "gtv 1", "Gtv 1"):
        one = rtstruct.select(cs, name)
        assert one.names == ["GTV 1"] and len(one.contours[0]) == 3
    assert rtstruct.select(cs, "BODY").names == ["Body"]
    with pytest.raises(ConfigurationError, match="'Body', 'GTV 1'.*mask_roi"):
        rtstruct.select(cs, None)                                                       # several ROIs and no name
    with pytest.raises(ConfigurationError, match="no ROI named 'GTV'.*'Body', 'GTV 1'"):
        rtstruct.select(cs, "GTV")                                                      # exact, not a prefix
    single = rtstruct.read(_write(tmp_path / "one.dcm", C.rtstruct_file(_two_rois()[1:])))
    assert rtstruct.select(single, None).names == ["GTV 1"] and rtstruct.select(rtstruct.select(cs, "gtv 1"), None).names == ["GTV 1"]
    with pytest.raises(ConfigurationError, match="no ROI named"):
        rtstruct.select(single, "Body")


def test_contours_arrive_sorted_by_slice_whatever_their_order_in_the_file(tmp_path):
    cs = rtstruct.select(rtstruct.read(_write(tmp_path / "s.dcm", C.rtstruct_file(_two_rois()))), "GTV 1")
    points, contours, slice_first, dropped = rtstruct.to_scan_index(cs, (6, 6, 4), C.LPS_AFFINE)
    assert points.dtype == np.float64 and contours.dtype == np.int32 and slice_first.dtype == np.int32 and dropped == {}
    assert slice_first.tolist() == [0, 1, 1, 3, 3] and contours.tolist() == [[0, 4], [4, 4], [8, 4]]
    # slice 0 holds the file's second contour; slice 2 the first and the third, in the file's order
    assert np.array_equal(points[0:4], C.square(0, 0.5, 2.25)[:, :2]) and np.array_equal(points[4:8], C.square(2)[:, :2])
    assert np.array_equal(points[8:12], C.square(2, 2.0, 3.0)[:, :2])
    mask, _, _ = C.fill_ref(points, contours, slice_first, (6, 6, 4))
    want = np.zeros((6, 6, 4), dtype=np.uint8)
    want[1:3, 1:3, 0] = 1                                                                # i < 2.25 and 0.5 <= j < 2.25
    want[1:4, 1:4, 2] = 1                                                                # the square [1, 4): the left edge is in, the right out
    want[2, 2, 2] = 0                                                                    # the inner square [2, 3) is a hole by even-odd
    assert np.array_equal(mask, want)


def test_a_contour_off_the_scans_slice_planes_is_refused(tmp_path):
    tilted = C.square(1)
    tilted[2:, 2] += 0.6                                                                 # 0.3 slice at 2 mm per slice
    path = _write(tmp_path / "o.dcm", C.rtstruct_file([("GTV", [("CLOSED_PLANAR", C.square(0), None), ("CLOSED_PLANAR", tilted, None)])]))
    with pytest.raises(ConfigurationError, match=r"o\.dcm: contour 1 of ROI 'GTV' spreads 0\.3 slices.*Export the structure set on the scan"):
        rtstruct.to_scan_index(rtstruct.read(path), (6, 6, 4), C.LPS_AFFINE)
    level = C.square(1)
    level[2:, 2] += 0.4                                                                  # 0.2 slice: within the bound; mean 1.1 -> slice 1
    path = _write(tmp_path / "l.dcm", C.rtstruct_file([("GTV", [("CLOSED_PLANAR", level, None)])]))
    assert rtstruct.to_scan_index(rtstruct.read(path), (6, 6, 4), C.LPS_AFFINE)[2].tolist() == [0, 0, 1, 1, 1]
    with pytest.raises(ConfigurationError, match="no geometry"):
        rtstruct.to_scan_index(rtstruct.read(path), (6, 6, 4), None)


def test_dropped_contours_are_counted_and_reported_once_per_file(tmp_path, caplog):
    contours = [("POINT", C.square(1)[:1], None), ("OPEN_PLANAR", C.square(1), None), ("OPEN_NONPLANAR", C.square(1), None),
                ("CLOSED_PLANAR", C.square(1)[:2], None), ("CLOSED_PLANAR", C.square(9), None), ("CLOSED_PLANAR", C.square(-1), None),
                ("CLOSED_PLANAR", C.square(3), None)]
    path = _write(tmp_path / "d.dcm", C.rtstruct_file([("GTV", contours)]))
    cs = rtstruct.read(path)
    assert cs.dropped == [{"POINT": 1, "OPEN_PLANAR": 1, "OPEN_NONPLANAR": 1, "fewer than 3 points": 1}] and len(cs.contours[0]) == 3
    with caplog.at_level(logging.WARNING, logger="mmnn_sts_amd.data.rtstruct"):
        first = rtstruct.to_scan_index(cs, (6, 6, 4), C.LPS_AFFINE)
        second = rtstruct.to_scan_index(cs, (6, 6, 4), C.LPS_AFFINE)
    assert first[3] == second[3] == {"POINT": 1, "OPEN_PLANAR": 1, "OPEN_NONPLANAR": 1, "fewer than 3 points": 1, "slice outside the scan": 2}
    assert first[2].tolist() == [0, 0, 0, 0, 1] and first[1].tolist() == [[0, 4]]
    warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "d.dcm" in warnings[0] and "OPEN_PLANAR" in warnings[0] and "slice outside the scan" in warnings[0]
    nothing = _write(tmp_path / "n.dcm", C.rtstruct_file([("GTV", contours[:6])]))
    with pytest.raises(ConfigurationError, match="ROI 'GTV' leaves nothing"):
        rtstruct.to_scan_index(rtstruct.read(nothing), (6, 6, 4), C.LPS_AFFINE)


def test_malformed_files_are_refused(tmp_path):
    path = _write(tmp_path / "count.dcm", C.rtstruct_file([("GTV", [("CLOSED_PLANAR", C.square(1), 5)])]))
    with pytest.raises(ConfigurationError, match="NumberOfContourPoints 5 .* holds 4 points"):
        rtstruct.read(path)
    e = lambda g, n, vr, v: D.el(g, n, vr, v, True)
    broken = C.sequence(0x3006, 0x0039, [e(0x3006, 0x0040, "SQ", b"") + e(0x3006, 0x0084, "IS", "99")])
    with pytest.raises(ConfigurationError, match="refers to ROINumber 99"):
        rtstruct.read(_write(tmp_path / "ref.dcm", C.rtstruct_file([("GTV", [])], extra=broken)))
    triplets = C.rtstruct_file([("GTV", [("CLOSED_PLANAR", C.square(1), None)])]).replace(b"\\2.0\\4.0\\", b"\\2.0 4.0 ", 1)
    with pytest.raises(ConfigurationError, match="malformed"):
        rtstruct.read(_write(tmp_path / "ds.dcm", triplets))
    image = D.part10(D.image_elements(), D.slice_bytes(3, 4, "i2")[1])
    with pytest.raises(ConfigurationError, match="is not RT Structure Set Storage"):
        rtstruct.read(_write(tmp_path / "image.dcm", image))
    from mmnn_sts_amd.data.dicom import NotDicomError
    with pytest.raises(NotDicomError):
        rtstruct.read(_write(tmp_path / "text.dcm", b"no magic here " * 20))
    with pytest.raises(ConfigurationError, match="DICOM SEG is outside the path"):
        rtstruct.read(_write(tmp_path / "seg.dcm", C.rtstruct_file(_two_rois(), sop_class="1.2.840.10008.5.1.4.1.1.66.4")))


@pytest.mark.parametrize("syntax,reason", [("1.2.840.10008.1.2.2", "big endian"), ("1.2.840.10008.1.2.1.99", "deflated"),
                                           ("1.2.840.10008.1.2.4.70", "encapsulated")])
def test_syntax_refusals_hold(tmp_path, syntax, reason):
    with pytest.raises(ConfigurationError, match=reason):
        rtstruct.read(_write(tmp_path / "x.dcm", C.rtstruct_file(_two_rois(), syntax=syntax)))


def test_nesting_beyond_max_depth_is_refused(tmp_path):
    from mmnn_sts_amd.data.dicom import MAX_DEPTH
    deep = D.el(0x0008, 0x1155, "UI", "1.2")
    for _ in range(MAX_DEPTH + 2):
        deep = C.sequence(0x0008, 0x1140, [deep], True, True)
    with pytest.raises(ConfigurationError, match="nested deeper"):
        rtstruct.read(_write(tmp_path / "deep.dcm", C.rtstruct_file(_two_rois(), extra=deep)))


# ---- the run-rectangle round trip on an oblique geometry ---------------------------------------------------------------------------------
OBLIQUE = G.affine((("z", 0.35), ("x", -0.5), ("y", 0.8)), (0.7, 0.9, 3.3), (-41.3, 22.7, -13.9))


@pytest.mark.parametrize("explicit,undefined", [(True, False), (False, True)])
def test_run_rectangles_come_back_as_the_mask(tmp_path, explicit, undefined):
    mask = (np.random.default_rng(12).random((37, 29, 6)) < 0.45).astype(np.uint8)
    mask[:, :, 3] = 0                                                                    # a slice without contours
    mask[0, :, 0] = mask[-1, :, 0] = 1                                                   # runs that touch the grid's first and last column
    path = synth_dicom.write_rtstruct(tmp_path / "m" / "rs.dcm", mask, OBLIQUE, "GTV", ("Body",), explicit, undefined)
    cs = rtstruct.read(path)
    assert cs.names == ["Body", "GTV"]
    one = rtstruct.select(cs, "gtv")
    points, contours, slice_first, dropped = rtstruct.to_scan_index(one, mask.shape, OBLIQUE)
    assert dropped == {} and slice_first[3] == slice_first[4] and slice_first[-1] == len(contours) == len(one.contours[0])
    assert (np.diff(slice_first) >= 0).all() and (contours[:, 1] == 4).all() and np.array_equal(contours[:, 0], 4 * np.arange(len(contours)))
    # the package's placement against the term-by-term restatement: fp64 products of coordinates below 1e3 mm err by ~1e-13
    ref = np.concatenate([C.index_ref(c, OBLIQUE) for c in one.contours[0]], axis=0)
    order = np.argsort(np.rint(ref[::4, 2]), kind="stable")
    assert np.abs(points - ref.reshape(-1, 4, 3)[order].reshape(-1, 3)[:, :2]).max() <= 1e-9
    got, near_x, near_row = C.fill_ref(points, contours, slice_first, mask.shape)
    print(f"smallest |xc - i| {near_x!r}, smallest vertex-to-row distance {near_row!r}")
    assert near_x >= 0.49 and near_row >= 0.49                                           # corners at half-integers, to the decimal strings' 1e-10
    assert np.array_equal(got, mask)
    decoy, _, _ = C.fill_ref(*rtstruct.to_scan_index(rtstruct.select(cs, "Body"), mask.shape, OBLIQUE)[:3], mask.shape)
    assert decoy[:, :, 0].all() and not decoy[:, :, 1:].any()


# ---- datasets ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("rt")
    synth_nifti.write_tree(root / "nifti", n_patients=3, seed=11, extent=((8, 12), (8, 12), (4, 6)))
    return synth_dicom.from_nifti_tree(root / "nifti", root / "dicom", mask_format="rtstruct", extra_rois=("Body",))


def _dataset(tree, **kw):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"], **kw)


def test_a_tree_with_rtstruct_masks_is_detected_and_constructs(tree):
    from mmnn_sts_amd.data import dicom
    ds = _dataset(tree, mask_roi="gtv")
    assert ds.layout == "dicom" and len(ds) == 3 and ds.other_grid == []
    raw = ds[0][0]
    assert len(raw.volumes) == 2
    for scan, mask in raw.volumes:
        assert isinstance(scan, dicom.DicomSeries) and isinstance(mask, rtstruct.ContourSet)
        assert mask.names == ["GTV"] and len(mask.contours[0]) > 0 and os.path.basename(mask.path) == "rtstruct.dcm"


def test_a_wrong_mask_roi_fails_at_construction_with_the_names(tree):
    with pytest.raises(ConfigurationError, match="no ROI named 'tumour'.*'Body', 'GTV'"):
        _dataset(tree, mask_roi="tumour")
    with pytest.raises(ConfigurationError, match="2 ROIs \\('Body', 'GTV'\\).*mask_roi"):
        _dataset(tree)


def test_parser_hands_mask_roi_to_the_datasets(tree):
    import argparse
    from mmnn_sts_amd.parser.parser import Parser
    p = Parser()
    p.parseConfig()
    p.config["Data"] = dict({k: tree[k] for k in ("image_loc", "key_loc", "data_loc")}, t1_path="t1", t2_path="t2", mask_roi="GTV")
    args = argparse.Namespace(classification=False, survival=True, images=True, preop=False, postop=False)
    ds = p.getDatasets(args, p.getImagePath())
    assert ds.mask_roi == "GTV" and p.image_layout == "dicom"
    p.config["Data"]["mask_roi"] = 7
    with pytest.raises(ConfigurationError, match="mask_roi"):
        p.getDatasets(args, p.getImagePath())
    p.config["Data"]["mask_roi"] = "nothing"
    with pytest.raises(ConfigurationError, match="no ROI named 'nothing'"):
        p.getDatasets(args, p.getImagePath())


def test_mask_directories_that_mix_are_refused(tree, tmp_path):
    import shutil
    from mmnn_sts_amd.data.ImageDatasets import rtstruct_in
    patient = os.path.join(tree["image_loc"], "t1", sorted(os.listdir(os.path.join(tree["image_loc"], "t1")))[0])
    rs = os.path.join(patient, "mask", "rtstruct.dcm")
    assert rtstruct_in(os.path.join(patient, "mask")) == rs and rtstruct_in(os.path.join(patient, "image")) is None
    two = tmp_path / "two" / "mask"
    os.makedirs(two)
    shutil.copyfile(rs, two / "a.dcm")
    shutil.copyfile(rs, two / "b.dcm")
    with pytest.raises(ConfigurationError, match="2 RTSTRUCT files"):
        rtstruct_in(two)
    mixed = tmp_path / "mixed" / "mask"
    os.makedirs(mixed)
    shutil.copyfile(rs, mixed / "rs.dcm")
    series = os.path.join(patient, "image", "series_1")
    shutil.copyfile(os.path.join(series, sorted(os.listdir(series))[0]), mixed / "slice.dcm")
    with pytest.raises(ConfigurationError, match="beside 1 DICOM image file"):
        rtstruct_in(mixed)
    sub = tmp_path / "sub" / "mask" / "RS_1"                                            # its single sub-directory
    os.makedirs(sub)
    shutil.copyfile(rs, sub / "rs.dcm")
    assert rtstruct_in(tmp_path / "sub" / "mask") == str(sub / "rs.dcm")


def test_a_contour_mask_beside_a_nifti_scan_is_refused(tree):
    from mmnn_sts_amd.data import ingest, nifti
    ds = _dataset(tree, mask_roi="gtv")
    contours = ds[0][0].volumes[0][1]
    scan = nifti.NiftiImage(np.zeros((8, 8, 4), dtype=np.int16), 4, 1.0, 0.0, "scan.nii", np.eye(4))
    with pytest.raises(ConfigurationError, match="RTSTRUCT mask beside a NIfTI scan"):
        ingest.mask_index_map(scan, contours)
    assert ingest.mask_index_map(ds[0][0].volumes[0][0], contours) is None


# ---- mmnn_rasterize_contours refuses bad arguments before any launch (no GPU: the pointers are fake and never dereferenced) ---------------
@pytest.fixture(scope="module")
def lib():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


P, R, S, O = 0x7F0000100000, 0x7F0000200000, 0x7F0000300000, 0x7F0000900000
_GOOD = dict(x=8, y=4, z=2, n_contours=3, n_points=12)
_BAD_CALLS = {
    "zero extent": (dict(y=0), P, R, S, O, "non-positive extent"), "negative extent": (dict(z=-3), P, R, S, O, "non-positive extent"),
    "x above the ingest's": (dict(x=2049), P, R, S, O, "x extent 2049 above 2048"),
    "negative n_contours": (dict(n_contours=-1), P, R, S, O, "n_contours"), "negative n_points": (dict(n_points=-1), P, R, S, O, "n_points"),
    "null points": ({}, 0, R, S, O, "null"), "null contours": ({}, P, 0, S, O, "null"), "null slice_first": ({}, P, R, 0, O, "null"),
    "null out": ({}, P, R, S, 0, "null"), "null slice_first without contours": (dict(n_contours=0, n_points=0), 0, 0, 0, O, "null"),
    "points misaligned": ({}, P + 4, R, S, O, "not aligned"), "contours misaligned": ({}, P, R + 2, S, O, "not aligned"),
}


@pytest.mark.parametrize("name", sorted(_BAD_CALLS))
def test_rasterize_contours_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    fields, points, contours, slice_first, out, reason = _BAD_CALLS[name]
    desc = _lib.RasterizeDesc(**dict(_GOOD, **fields))
    assert lib.mmnn_rasterize_contours(ctypes.byref(desc), points or None, contours or None, slice_first or None, out or None, None) == 1
    with pytest.raises(ValueError, match=reason):
        _lib.check(1, "mmnn_rasterize_contours")


def test_rasterize_contours_refuses_a_null_descriptor_and_exports_the_chunk(lib):
    from mmnn_sts_amd import _lib
    assert lib.mmnn_rasterize_contours(None, P, R, S, O, None) == 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmnn_sts.h")).read()
    assert f"#define MMNN_RASTERIZE_CHUNK_EDGES {_lib.RASTERIZE_CHUNK_EDGES}\n" in header
