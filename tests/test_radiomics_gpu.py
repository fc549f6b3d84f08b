"""`mmnn_radiomics` on the device against the numpy restatement (tests/_radiomics_ref.py), `radiomics.extract` through every mask
route, the MLP at the radiomic input width, and the command lines in fresh processes.

Everything integer or selected is compared with array equality: n, the bounding box, the nine index moments, Ng, the histogram, the 13
matrices, the ten order statistics; the interpolated percentiles, Minimum, Maximum and Range bitwise.  The other fp64 features are held to
tests/_radiomics_cases.py: BOUND, relative to the scale the restatement returns beside each value; the restatement itself is asserted to
stay within MEASURED against the mpmath evaluation for every case, so no case goes unchecked."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import ingest, synth_dicom, synth_nifti
from tests import _radiomics_ref as R
from tests._radiomics_cases import BOUND, CASES, MEASURED
from tests._radiomics_harness import DEV, ROOT, cut, first_call, mlp_at_width, process
from tests._cli import tiny_config

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(name):
    """The restatement of a case, computed once and shared."""
    if name not in _REF:
        c = CASES[name]
        with np.errstate(all="ignore"):
            ref = R.restate(c["scan"], c["mask"], c["bin_width"], c["max_bins"], c["scan_scale"], c["mask_scale"])
        ref["exact"] = None if (ref["empty"] or ref["nonfinite"] or ref["overflow"]) else R.exact(ref)
        _REF[name] = ref
    return _REF[name]


def _run(name):
    """One call through the C-ABI itself: result block, hist and glcm sit between guard bytes inside one buffer; returns
    (fields, hist, glcm) on the host."""
    mb = CASES[name]["max_bins"]
    _, _, buf, offs, sizes = first_call(CASES[name], guard=True)
    torch.cuda.synchronize()
    block, hist, glcm = cut(buf, offs, sizes, f"{name}: bytes outside result / hist / glcm were written")
    return radiomics.unpack_block(block), hist.view(np.uint32).astype(np.int64), glcm.view(np.uint32).astype(np.int64).reshape(13, mb, mb), block


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _compare(name):
    ref = _ref(name)
    fields, hist, glcm, _ = _run(name)
    assert fields["n"] == ref["n"], name
    assert np.array_equal(fields["lo"], ref["lo"]) and np.array_equal(fields["hi"], ref["hi"]), (name, fields["lo"], fields["hi"], ref["lo"], ref["hi"])
    assert np.array_equal(fields["moments"], ref["moments"]), name
    assert (fields["empty"], fields["nonfinite"], fields["overflow"]) == (ref["empty"], ref["nonfinite"], ref["overflow"]), name
    assert np.array_equal(hist, ref["hist"]), name
    assert np.array_equal(glcm, ref["glcm"]), (name, int(np.abs(glcm - ref["glcm"]).sum()))
    if ref["empty"] or ref["nonfinite"] or ref["overflow"]:
        assert fields["n_bins"] == ref["n_bins"]
        assert np.isnan(fields["order"]).all() and np.isnan(fields["firstorder"]).all() and np.isnan(fields["glcm"]).all(), name
        return fields, ref
    assert fields["n_bins"] == ref["n_bins"], name
    assert _same_bits(fields["order"], ref["order"]), (name, fields["order"], ref["order"])
    got = dict(zip(R.FIRSTORDER, fields["firstorder"]))
    got.update(zip(R.GLCM, fields["glcm"]))
    for k in R.BITWISE:
        assert _same_bits(got[k], ref["firstorder"][k][0]), (name, k, got[k], ref["firstorder"][k][0])
    values = {k: R.value_and_scale(ref, k)[0] for names in R.CLASSES.values() for k in names}
    own = R.deviations(ref, values, ref["exact"])
    dev = R.deviations(ref, {k: float(got[k]) for k in values}, ref["exact"])
    print(name, "restatement", {k: f"{v / 2 ** -53:.2f}" for k, v in own.items()}, "device", {k: f"{v / 2 ** -53:.2f}" for k, v in dev.items()})
    for cls in R.CLASSES:
        assert own[cls] <= MEASURED[cls], (name, cls, "restatement", own[cls] / 2 ** -53)
        assert dev[cls] <= BOUND[cls], (name, cls, "device", dev[cls] / 2 ** -53,
                                        {k: (float(got[k]), values[k]) for k in R.CLASSES[cls]})
    return fields, ref


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("scan_")])
def test_against_restatement(name):
    fields, ref = _compare(name)
    if name == "single_voxel":
        assert fields["n"] == 1 and np.isnan(fields["glcm"]).all() and np.isfinite(fields["firstorder"]).all()
    if name == "global_ng240":
        assert fields["n_bins"] == 240                   # above the 128 x 128 matrix that the LDS variant holds
    if name == "overflow":
        assert fields["overflow"] and fields["n_bins"] == 1200
    if name == "nan_outside":
        assert not fields["nonfinite"]
    if name == "n2":
        assert math.isnan(fields["firstorder"][R.FIRSTORDER.index("RobustMeanAbsoluteDeviation")])   # no value inside [p10, p90]


@pytest.mark.parametrize("dtype", [n[5:] for n in CASES if n.startswith("scan_")])
def test_scan_types_with_scaled_mask_and_negative_slope(dtype):
    fields, ref = _compare(f"scan_{dtype}")
    c = CASES[f"scan_{dtype}"]
    assert 0 < fields["n"] < int((c["mask"] != 0).sum()) + int((c["mask"] == 0).sum())
    assert ref["n"] == int((c["mask"] != 3).sum())       # raw 3 scales to 0: outside; raw 0 scales to -6: inside


@pytest.mark.parametrize("name", ["ellipsoid", "global_ng240", "whole_volume_vec4"])
def test_two_calls_agree_bit_for_bit(name):
    a, b = _run(name), _run(name)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_refusals():
    L = _lib.lib()
    assert L.mmnn_radiomics_workspace_bytes(0, 4, 4, 256) == -1
    assert L.mmnn_radiomics_workspace_bytes(4, 4, 4, 0) == -1 and L.mmnn_radiomics_workspace_bytes(4, 4, 4, _lib.RADIOMICS_MAX_BINS + 1) == -1
    t = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for bad in (dict(bin_width=0.0), dict(bin_width=float("nan")), dict(scan_type=3), dict(mask_type=1)):
        kw = dict(x=4, y=4, z=4, scan_type=4, mask_type=2, scan_slope=1.0, scan_inter=0.0, mask_slope=1.0, mask_inter=0.0, bin_width=25.0, max_bins=16)
        kw.update(bad)
        desc = _lib.RadiomicsDesc(**kw)
        p = t.data_ptr()
        assert L.mmnn_radiomics(ctypes.byref(desc), p, p + 1024, p + 2048, p + 4096, p + 8192, p + 32768, None) == 1, bad


# ---- the MLP at the radiomic widths ----------------------------------------------------------------------------------------------------
# input stream per width: the first index at which no pre-activation of the fp64 reference is within 1e-4 of zero (found on the CPU)
MLP_STREAM = {47: 0, 94: 0, 126: 0}


@pytest.mark.parametrize("width", [47, 94, 126])
def test_mlp_at_radiomic_width_vs_fp64(width):
    """tests/_radiomics_harness.py: mlp_at_width, at the three widths of the default table."""
    mlp_at_width(width, MLP_STREAM[width])


# ---- extract through every mask route ------------------------------------------------------------------------------------------------------
def _dataset(tree, **kw):
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    return ImageDataset(os.path.join(tree["image_loc"], "t1"), tree["key_loc"], **kw)


def _integers(ds, threshold=None):
    """Per patient: the integer outputs of extract, and those of the restatement on the scan's raw voxels and the mask that the shared
    front (`ingest.prepare_pair`) put on the scan's grid."""
    out = []
    for p in ds.patients:
        scan, mask = ds._load(p)
        res = radiomics.extract(scan, mask, DEV, threshold=threshold)
        sd, md = ingest.prepare_pair(scan, mask, torch.device(DEV), None, threshold)
        torch.cuda.synchronize()
        f = radiomics.unpack_block(res.block.cpu().numpy())
        assert not (f["empty"] or f["nonfinite"] or f["overflow"]) and f["n"] > 0
        x, y, z = sd.shape
        dt = {v: k for k, v in ingest.TYPE_CODES.items()}
        sraw = sd.data.cpu().numpy().view(dt[sd.datatype]).reshape((x, y, z), order="F")
        mraw = md.data.cpu().numpy().view(dt[md.datatype]).reshape((x, y, z), order="F")
        ref = R.restate(sraw, mraw, 25.0, 256, (sd.slope, sd.inter), (md.slope, md.inter))
        got = (f["n"], f["lo"], f["hi"], f["moments"], f["n_bins"], res.hist.cpu().numpy().astype(np.int64), res.glcm.cpu().numpy().astype(np.int64))
        want = (ref["n"], ref["lo"], ref["hi"], ref["moments"], ref["n_bins"], ref["hist"], ref["glcm"])
        for g, w in zip(got, want):
            assert np.array_equal(g, w), p
        assert _same_bits(f["order"], ref["order"])
        feats = radiomics.finish(res)
        assert list(feats) == list(radiomics.FEATURE_NAMES) and all(math.isfinite(v) for v in feats.values())
        out.append(got)
    return out


def test_extract_through_each_mask_route(tmp_path):
    from tests.test_rtstruct_gpu import _with_geometry
    ntree = synth_nifti.write_tree(tmp_path / "nifti", n_patients=2, seed=5)
    _with_geometry(ntree, 2)
    same = _integers(_dataset(ntree))
    twins = {}
    for fmt in ("series", "rtstruct", "seg"):
        dtree = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / f"dicom_{fmt}", seed=5, mask_format=fmt)
        twins[fmt] = _integers(_dataset(dtree))
    for fmt, rows in twins.items():
        for a, b in zip(same, rows):
            for g, w in zip(a, b):
                assert np.array_equal(g, w), fmt                 # the DICOM twins give the NIfTI tree's integers exactly
    own = synth_nifti.write_tree(tmp_path / "own", n_patients=2, seed=5, mask_grid="own")
    _integers(_dataset(own))


def test_finish_raises_with_the_cause():
    from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
    c = CASES["overflow"]
    res = radiomics.extract(c["scan"], c["mask"], DEV, bin_width=5.0)
    with pytest.raises(ConfigurationError, match="bin_width"):
        radiomics.finish(res, None)
    c = CASES["empty"]
    with pytest.raises(ConfigurationError, match="no voxel"):
        radiomics.finish(radiomics.extract(c["scan"], c["mask"], DEV), None)
    c = CASES["nan_inside"]
    with pytest.raises(ConfigurationError, match="NaN"):
        radiomics.finish(radiomics.extract(c["scan"], c["mask"], DEV), None)
    c = CASES["ellipsoid"]
    first = radiomics.extract(c["scan"], c["mask"], DEV)
    again = radiomics.extract(c["scan"], c["mask"], DEV, buffers=first)
    assert again.block.data_ptr() == first.block.data_ptr()
    feats = radiomics.finish(again, np.diag([0.5, 2.0, 3.0, 1.0]))
    ref = R.shape_reference(c["mask"] != 0, np.diag([0.5, 2.0, 3.0]))
    for k, v in ref.items():
        assert feats[f"original_shape_{k}"] == pytest.approx(v, rel=1e-12)
    assert feats["original_firstorder_TotalEnergy"] == pytest.approx(feats["original_firstorder_Energy"] * 3.0, rel=1e-14)


# ---- the command lines: one fresh process each -----------------------------------------------------------------------------------------------
def test_cli_extraction_tool_writes_the_rows_of_finish(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=4, seed=11)
    out = tmp_path / "radiomics.csv"
    process(["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--out", str(out)], tmp_path)
    cols, rows = radiomics.read_csv(out)
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in radiomics.FEATURE_NAMES] and len(rows) == 4
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    for px in ("t1", "t2"):
        ds = ImageDataset(os.path.join(tree["image_loc"], px), tree["key_loc"])
        for p in ds.patients:
            want = radiomics.finish(radiomics.extract(*ds._load(p), DEV))
            row = next(r for r in rows if int(r[0]) == ds._uid_of(p))
            for n, v in want.items():
                assert float(row[cols.index(f"{px}_{n}")]) == v, (p, n)


def test_cli_trains_on_extracted_features_then_infers_with_images(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=12, val_fraction=0.34)
    loc = ["--config", tiny_config(tmp_path), "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = process([main, "--output_path", str(out), "--radiomics", "--survival", "--image_loc", tree["image_loc"], "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    for name in ("radiomics_features.csv", "radiomics_scaler.csv", "best_surv_model.pth"):
        assert (out / name).exists(), name
    out2 = tmp_path / "run2"
    out2.mkdir()
    rad = ["--rad_loc", str(out / "radiomics_features.csv"), "--image_loc", tree["image_loc"]]
    process([main, "--output_path", str(out2), "--radiomics", "--images", "--survival", "--epochs", "1", *rad, *loc], out2)
    log = process([main, "--output_path", str(out2), "--inference", "--radiomics", "--images", "--survival", "--weights",
                    str(out2 / "best_surv_model.pth"), *rad, *loc], out2)
    assert "All C-indexes" in log
