"""`mmnn_radiomics_mesh` on the device against the numpy restatement (tests/_radiomics_mesh_ref.py), the mesh switch through
`radiomics.extract` / `finish` / `extract_tree` / the command lines, and the MLP at the widths the wider table brings.

cfg, the three integers and the four squared diameters are compared exactly / bitwise.  SurfaceArea is held to BOUND of
tests/_radiomics_mesh_cases.py (64 * 2^-53, the floor; 8 x the restatement's measured 5.99 * 2^-53 is below it) relative to the sum, against the mpmath
evaluation of the same integer normals; the NaN / zero pattern of the flagged cases is exact."""
import ctypes
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import ingest, synth_nifti
from tests import _radiomics_mesh_ref as M
from tests import _radiomics_ref as R
from tests._radiomics_harness import (DEV, GOOD_DESC, GUARD, ROOT, cut, first_call, follow_call, leave_the_dropout_stream_where_it_was,  # noqa: F401
                                      mlp_at_width, process, refusal_walk)
from tests._cli import tiny_config
from tests._radiomics_mesh_cases import BOUND, FLAGGED, MESH_CASES, MLP_STREAM, OBLIQUE, U

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(name):
    """The restatement of a case, computed once and shared."""
    if name not in _REF:
        c = MESH_CASES[name]
        _REF[name] = M.restate(R.scaled(c["mask"], *c["mask_scale"]) != 0.0, c["L"], flagged=name in FLAGGED)
    return _REF[name]


def _run(name):
    """mmnn_radiomics, then mmnn_radiomics_mesh through the C-ABI itself: the result block and cfg sit between guard bytes inside one
    buffer filled with a pattern; both workspaces start from 0xFF.  Returns dict(block, cfg (bytes), fields (of the first call))."""
    c = MESH_CASES[name]
    sizes = [_lib.RADIOMICS_MESH_BYTES, _lib.RADIOMICS_MESH_CONFIGS * 8]
    r, desc, first, _, _ = first_call(c)
    r.linear = np.eye(3) if c["L"] is None else c["L"]
    buf, offs, ws4, n4 = follow_call(r, desc, "mesh", sizes, behind=GUARD)
    torch.cuda.synchronize()
    block, cfg = cut(buf, offs, sizes, f"{name}: bytes outside the mesh block and cfg were written")
    assert (ws4[n4:] == 0xFF).all(), f"{name}: bytes behind the mesh workspace were written"
    return {"block": block, "cfg": cfg, "fields": radiomics.unpack_block(first[:_lib.RADIOMICS_RESULT_BYTES].cpu().numpy())}


@pytest.mark.parametrize("name", list(MESH_CASES))
def test_against_restatement(name):
    ms, got = _ref(name), _run(name)
    dev, cfg = radiomics.unpack_mesh(got["block"]), got["cfg"].view(np.uint64).astype(np.int64)
    flagged = got["fields"]["empty"] or got["fields"]["nonfinite"] or got["fields"]["overflow"]
    assert flagged == (name in FLAGGED)
    assert np.array_equal(cfg, ms["cfg"]), (name, np.flatnonzero(cfg != ms["cfg"])[:8])
    assert {k: dev[k] for k in M.INTEGERS} == {k: ms[k] for k in M.INTEGERS}, name
    if name in FLAGGED:
        assert math.isnan(dev["area"]) and np.isnan(dev["q"]).all() and not cfg.any() and not any(dev[k] for k in M.INTEGERS)
        return
    assert dev["q"].view(np.uint64).tolist() == ms["q"].view(np.uint64).tolist(), (name, dev["q"], ms["q"])      # bit for bit
    own, mine = M.area_deviation(ms["area"], ms["cfg"], ms["L"]), M.area_deviation(dev["area"], ms["cfg"], ms["L"])
    print(name, "V", dev["n_vertices"], "area deviation / 2^-53: restatement", f"{own / U:.2f}", "device", f"{mine / U:.2f}")
    assert math.isfinite(dev["area"]) and mine <= BOUND, (name, mine / U, dev["area"], ms["area"])


@pytest.mark.parametrize("name", ["ellipsoid_24", "ellipsoid_24_oblique", "all_configs", "line_1x1x300", "box_v258", "checkerboard"])
def test_two_calls_agree_bit_for_bit(name):
    a, b = _run(name), _run(name)
    for k in ("block", "cfg"):
        assert np.array_equal(a[k], b[k]), (name, k)


def test_refusals_write_nothing():
    L = _lib.lib()
    t = torch.zeros(1 << 17, dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    lin = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    ptrs = [p, p + 65536, p + 1024, p + 2048, p + 32768]          # result, ws, out, cfg, ws4
    call = lambda desc, q, linear=lin: L.mmnn_radiomics_mesh(desc, q[0], q[1], linear, q[2], q[3], q[4], None)
    desc = ctypes.byref(_lib.RadiomicsDesc(**GOOD_DESC))
    assert call(desc, ptrs, None) == 1 and "null" in _lib.last_error()
    assert call(desc, ptrs, (ctypes.c_double * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)) == 1 and "linear[4]" in _lib.last_error()
    refusal_walk(call, ptrs, ((0, 4), (1, 64), (2, 4), (3, 4), (4, 64)), (dict(bin_width=0.0), dict(scan_type=3), dict(x=0), dict(max_bins=0)), t)


def _on_grid(arr, affine, slope=1.0, inter=0.0):
    return dataclasses.replace(ingest.upload(arr, torch.device(DEV), slope, inter), affine=affine)


def test_all_switches_on_is_each_switch_alone():
    c = MESH_CASES["seven_levels"]                          # (no header scaling, no lead: `extract` on the arrays sees what `_run` uploads)
    every = radiomics.TEXTURE_CLASSES
    plain = radiomics.extract(c["scan"], c["mask"], DEV)
    off = radiomics.extract(c["scan"], c["mask"], DEV, classes=every, glszm=True, mesh=False)
    tex = radiomics.extract(c["scan"], c["mask"], DEV, classes=every)
    zon = radiomics.extract(c["scan"], c["mask"], DEV, glszm=True)
    alone = radiomics.extract(c["scan"], c["mask"], DEV, mesh=True)
    wide = radiomics.extract(c["scan"], c["mask"], DEV, classes=every, glszm=True, mesh=True)
    for r in (plain, off, tex, zon):
        assert r.mesh is None and r.mesh_cfg is None and r.mesh_workspace is None and r.linear is None and r.mesh_shape is False
    assert wide.mesh_shape is True and alone.mesh_shape is True and alone.texture is None and alone.zones is None and alone.classes == ()
    assert np.array_equal(alone.linear, np.eye(3))
    for r in (off, tex, zon, alone, wide):                  # with the switch off or on, every other result is byte for byte what it was
        for k in ("block", "hist", "glcm"):
            assert torch.equal(getattr(r, k), getattr(plain, k)), k
    for r in (off, wide):
        for k in ("texture", "glrlm", "gldm", "ngtdm_n", "ngtdm_s"):
            assert torch.equal(getattr(r, k), getattr(tex, k)), k
        for k in ("zones", "labels", "sizes", "levels"):
            assert torch.equal(getattr(r, k), getattr(zon, k)), k
    assert torch.equal(wide.mesh, alone.mesh) and torch.equal(wide.mesh_cfg, alone.mesh_cfg)
    ms = _ref("seven_levels")
    assert np.array_equal(wide.mesh_cfg.cpu().numpy(), ms["cfg"])
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
    narrow, offf, texf, zonf, alonef, widef = (radiomics.finish(r, None) for r in (plain, off, tex, zon, alone, wide))
    assert list(narrow) == list(radiomics.FEATURE_NAMES) and list(offf) == list(radiomics.feature_names(every, True)) and len(offf) == 98
    assert list(alonef) == list(radiomics.feature_names(mesh=True)) and len(alonef) == 55
    assert list(widef) == list(radiomics.feature_names(every, True, True)) and len(widef) == 106
    for part in (narrow, offf, texf, zonf, alonef):
        assert all(same(widef[k], v) for k, v in part.items())
    want = M.derived(ms["volume48"], radiomics.unpack_mesh(wide.mesh.cpu().numpy())["area"], ms["q"], np.eye(3))
    assert [widef[f"original_shape_{n}"] for n in M.MESH_SHAPE] == pytest.approx([want[n] for n in M.MESH_SHAPE], rel=8 * U)
    assert widef["original_shape_Maximum3DDiameter"] == math.sqrt(ms["q"][0]) / 2.0 and all(math.isfinite(v) for v in alonef.values())
    with pytest.raises(ValueError, match="enqueued under"):
        radiomics.finish(wide, np.diag([2.0, 2.0, 2.0, 1.0]))
    again = radiomics.extract(c["scan"], c["mask"], DEV, mesh=True, buffers=wide)          # the buffers are written again
    assert again.mesh.data_ptr() == wide.mesh.data_ptr() and again.mesh_cfg.data_ptr() == wide.mesh_cfg.data_ptr()
    assert again.mesh_workspace.data_ptr() == wide.mesh_workspace.data_ptr() and all(same(v, alonef[k]) for k, v in radiomics.finish(again, None).items())


def test_extract_passes_the_scans_linear_part():
    c = MESH_CASES["ellipsoid_24_oblique"]
    aff = np.eye(4)
    aff[:3, :3], aff[:3, 3] = OBLIQUE, (-90.0, 126.0, -72.0)
    r = radiomics.extract(_on_grid(c["scan"], aff), _on_grid(c["mask"], aff), DEV, mesh=True)
    assert np.array_equal(r.linear, OBLIQUE)
    ms, dev = _ref("ellipsoid_24_oblique"), radiomics.unpack_mesh(r.mesh.cpu().numpy())
    assert dev["q"].view(np.uint64).tolist() == ms["q"].view(np.uint64).tolist() and dev["volume48"] == ms["volume48"]
    f = radiomics.finish(r)
    want = M.derived(ms["volume48"], dev["area"], ms["q"], OBLIQUE)
    assert [f[f"original_shape_{n}"] for n in M.MESH_SHAPE] == pytest.approx([want[n] for n in M.MESH_SHAPE], rel=8 * U)
    assert f["original_shape_MeshVolume"] < f["original_shape_VoxelVolume"] and radiomics.finish(r, aff) == f
    with pytest.raises(ValueError, match="enqueued under"):
        radiomics.finish(r, None)


# ---- the MLP at the wider tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", sorted(MLP_STREAM))
def test_mlp_at_mesh_width_vs_fp64(width):
    """MLP(width) forward and backward at N = 4, training mode, against the fp64 torch restatement, at the bar tests/test_tail_ops_gpu.py
    holds width 32 to: 106 columns of one modality with every switch on, 244 = 32 clinical columns + 2 x 106."""
    mlp_at_width(width, MLP_STREAM[width])


# ---- through the Python layer and the command lines ------------------------------------------------------------------------------------------
def test_extract_tree_and_the_extraction_tool_write_the_eight_columns_last(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=15)
    names = radiomics.feature_names((), False, True)
    ds = ImageDataset(os.path.join(tree["image_loc"], "t1"), tree["key_loc"])
    out = tmp_path / "t1.csv"
    part = radiomics.extract_tree(ds, DEV, str(out), mesh=True)
    assert list(part[0]) == ["MRN"] + list(names) and len(part[0]) == 56
    cols, rows = radiomics.read_csv(out)
    assert cols == ["MRN"] + list(names) and cols[-8:] == [f"original_shape_{n}" for n in M.MESH_SHAPE] and len(rows) == 3
    assert radiomics.extract_tree(ds, DEV)[0].keys() == {"MRN", *radiomics.FEATURE_NAMES}        # off: the table it was
    for p in ds.patients:
        scan, mask = ds._load(p)
        r = radiomics.extract(scan, mask, DEV, mesh=True)
        want = radiomics.finish(r)
        row = next(q for q in part if q["MRN"] == ds._uid_of(p))
        assert all(row[n] == v for n, v in want.items()) and all(math.isfinite(v) for v in want.values()), p
        # the device against the restatement on the patient's own ROI and affine
        roi = R.scaled(np.asarray(mask.raw), mask.slope, mask.inter) != 0.0 if hasattr(mask, "raw") else None
        if roi is not None and roi.shape == tuple(r.shape):
            ms, dev = M.restate(roi, r.linear), radiomics.unpack_mesh(r.mesh.cpu().numpy())
            assert dev["q"].view(np.uint64).tolist() == ms["q"].view(np.uint64).tolist() and [dev[k] for k in M.INTEGERS] == [ms[k] for k in M.INTEGERS]
            assert M.area_deviation(dev["area"], ms["cfg"], ms["L"]) <= BOUND
    # the command line, every switch on
    wide = radiomics.feature_names("all", True, True)
    out2 = tmp_path / "radiomics.csv"
    log = process(["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--classes", "all", "--glszm",
                    "--mesh_shape", "--out", str(out2)], tmp_path)
    assert "212 features" in log
    cols, rows = radiomics.read_csv(out2)
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in wide] and len(cols) == 1 + 2 * 106 and len(rows) == 3
    assert all(float(rows[k][cols.index("t1_" + n)]) == part[k][n] for k in range(3) for n in names)


def test_cli_trains_the_fusion_model_with_mesh_shape_then_infers(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=16, val_fraction=0.34)
    loc = ["--config", tiny_config(tmp_path, radiomics={"classes": list(radiomics.TEXTURE_CLASSES), "glszm": True, "mesh_shape": True}), "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"], "--image_loc", tree["image_loc"]]
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = process([main, "--output_path", str(out), "--radiomics", "--images", "--survival", "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    cols, rows = radiomics.read_csv(out / "radiomics_features.csv")
    assert len(cols) == 1 + 2 * 106 and cols[-1] == "t2_original_shape_Maximum2DDiameterRow" and len(rows) == 6
    assert cols[106] == "t1_original_shape_Maximum2DDiameterRow" and os.path.exists(out / "radiomics_scaler.csv")
    log = process([main, "--output_path", str(out), "--inference", "--radiomics", "--images", "--survival", "--weights",
                    str(out / "best_surv_model.pth"), "--rad_loc", str(out / "radiomics_features.csv"), *loc], out)
    assert "All C-indexes" in log
