"""`mmnn_radiomics_zones` on the device against the numpy / scipy restatement (tests/_radiomics_zones_ref.py), the size-zone switch through
`radiomics.extract` / `finish` / the command lines, and the MLP at the widths the wider table brings.

The labels, the sizes, the per-level counts and the six integers are compared with array equality.  The 16 fp64 features are held to
tests/_radiomics_zones_cases.py: BOUND relative to the scale the restatement returns beside each value, against the mpmath evaluation of the
same integer tables; the NaN / zero pattern of the flagged cases is exact."""
import math
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import synth_nifti
from tests import _radiomics_zones_ref as Z
from tests._radiomics_harness import (DEV, ROOT, cut, first_call, follow_call, leave_the_dropout_stream_where_it_was, mlp_at_width,  # noqa: F401
                                      process, refusal_walk)
from tests._cli import tiny_config
from tests._radiomics_zones_cases import BOUND, FLAGGED, MLP_STREAM, ZONE_CASES

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(name):
    """The restatement of a case and the mpmath evaluation of its tables, computed once and shared."""
    if name not in _REF:
        zn = Z.restate(ZONE_CASES[name])
        zn["exact"] = None if zn["flagged"] else Z.exact(zn)
        _REF[name] = zn
    return _REF[name]


def _run(name):
    """mmnn_radiomics, then mmnn_radiomics_zones through the C-ABI itself: the result block and the three tables sit between guard bytes
    inside one buffer filled with a pattern, and ws3 starts from 0xFF.  Returns dict(block (bytes of the zones block), labels, sizes, levels
    (int64), fields (of the first call))."""
    c = ZONE_CASES[name]
    mb, n = c["max_bins"], c["scan"].size
    sizes = [_lib.RADIOMICS_ZONES_BYTES, n * 4, n * 4, mb * 4]
    r, desc, first, _, _ = first_call(c)
    buf, offs, _, _ = follow_call(r, desc, "zones", sizes)
    torch.cuda.synchronize()
    got = cut(buf, offs, sizes, f"{name}: bytes outside the zones block and the tables were written")
    return {"block": got[0], "labels": got[1].view(np.uint32).astype(np.int64), "sizes": got[2].view(np.uint32).astype(np.int64),
            "levels": got[3].view(np.uint32).astype(np.int64), "fields": radiomics.unpack_block(first[:_lib.RADIOMICS_RESULT_BYTES].cpu().numpy())}


@pytest.mark.parametrize("name", list(ZONE_CASES))
def test_against_restatement(name):
    zn, got = _ref(name), _run(name)
    ref = zn["ref"]
    assert (got["fields"]["empty"], got["fields"]["nonfinite"], got["fields"]["overflow"]) == (ref["empty"], ref["nonfinite"], ref["overflow"])
    for k in ("labels", "sizes", "levels"):
        assert np.array_equal(got[k], zn[k]), (name, k, int((got[k] != zn[k]).sum()))
    dev_f = radiomics.unpack_zones(got["block"])
    assert {k: dev_f[k] for k in Z.INTEGERS} == zn["integers"], name
    if name in FLAGGED:
        assert zn["flagged"] and np.isnan(dev_f["glszm"]).all() and not any(got[k].any() for k in ("labels", "sizes", "levels"))
        assert not any(dev_f[k] for k in Z.INTEGERS)
        return
    values = dict(zip(Z.GLSZM, dev_f["glszm"]))
    assert all(math.isfinite(v) for v in values.values()), (name, values)
    own = Z.deviations(zn, {k: v[0] for k, v in zn["features"].items()}, zn["exact"])
    dev = Z.deviations(zn, values, zn["exact"])
    print(name, "restatement", {k: f"{v / 2 ** -53:.2f}" for k, v in own.items()}, "device", {k: f"{v / 2 ** -53:.2f}" for k, v in dev.items()})
    for cls in Z.CLASSES:
        assert dev[cls] <= BOUND[cls], (name, cls, "device", dev[cls] / 2 ** -53, values, zn["features"])


@pytest.mark.parametrize("name", ["ellipsoid", "serpentine", "noise_ng8", "run_ng300_l64", "big_zone"])
def test_two_calls_agree_bit_for_bit(name):
    a, b = _run(name), _run(name)
    for k in ("block", "labels", "sizes", "levels"):
        assert np.array_equal(a[k], b[k]), (name, k)


def test_refusals():
    L = _lib.lib()
    assert L.mmnn_radiomics_zones_workspace_bytes(0, 4, 4, 256) == -1 and L.mmnn_radiomics_zones_workspace_bytes(4, 4, -1, 256) == -1
    assert L.mmnn_radiomics_zones_workspace_bytes(4, 4, 4, 0) == -1
    assert L.mmnn_radiomics_zones_workspace_bytes(4, 4, 4, _lib.RADIOMICS_MAX_BINS + 1) == -1
    assert L.mmnn_radiomics_zones_workspace_bytes(2048, 2048, 512, 256) == -1          # 2^31 voxels
    assert "2^31" in _lib.last_error()
    assert 0 < L.mmnn_radiomics_zones_workspace_bytes(4, 4, 4, 16) <= 32768
    t = torch.zeros(1 << 17, dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    ptrs = [p, p + 65536, p + 1024, p + 2048, p + 4096, p + 8192, p + 32768]      # result, ws, out, labels, sizes, levels, ws3
    refusal_walk(lambda desc, q: L.mmnn_radiomics_zones(desc, *q, None), ptrs, ((0, 4), (1, 64), (2, 4), (3, 2), (4, 2), (5, 2), (6, 64)),
                 (dict(bin_width=0.0), dict(bin_width=float("nan")), dict(scan_type=3), dict(mask_type=1), dict(x=0), dict(max_bins=0),
                  dict(max_bins=_lib.RADIOMICS_MAX_BINS + 1)), t)


def test_without_the_switch_the_extraction_is_what_it_was():
    c = ZONE_CASES["seven_levels"]                          # (no header scaling, no lead: `extract` on the arrays sees what `_run` uploads)
    every = radiomics.TEXTURE_CLASSES
    plain = radiomics.extract(c["scan"], c["mask"], DEV)
    off = radiomics.extract(c["scan"], c["mask"], DEV, classes=every, glszm=False)
    tex = radiomics.extract(c["scan"], c["mask"], DEV, classes=every)
    wide = radiomics.extract(c["scan"], c["mask"], DEV, classes=every, glszm=True)
    alone = radiomics.extract(c["scan"], c["mask"], DEV, glszm=True)
    for r in (plain, off, tex):
        assert r.zones is None and r.labels is None and r.sizes is None and r.levels is None and r.zones_workspace is None and r.glszm is False
    assert wide.glszm is True and alone.glszm is True and alone.texture is None and alone.classes == ()
    for r in (off, tex, wide, alone):
        for k in ("block", "hist", "glcm"):
            assert torch.equal(getattr(r, k), getattr(plain, k)), k
    for r in (off, wide):
        for k in ("texture", "glrlm", "gldm", "ngtdm_n", "ngtdm_s"):
            assert torch.equal(getattr(r, k), getattr(tex, k)), k
    zn = _ref("seven_levels")
    assert np.array_equal(wide.labels.cpu().numpy().astype(np.int64), zn["labels"]) and torch.equal(wide.zones, alone.zones)
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
    narrow, texf, widef, alonef = (radiomics.finish(r, None) for r in (plain, tex, wide, alone))
    assert list(narrow) == list(radiomics.FEATURE_NAMES) and list(texf) == list(radiomics.feature_names(every)) and len(texf) == 82
    assert list(widef) == list(radiomics.feature_names(every, glszm=True)) and len(widef) == 98
    assert list(alonef) == list(radiomics.feature_names((), glszm=True)) and len(alonef) == 63
    assert all(same(widef[k], v) for k, v in texf.items()) and all(same(widef[k], v) for k, v in alonef.items())
    assert all(same(alonef[k], v) for k, v in narrow.items())
    assert [widef[f"original_glszm_{n}"] for n in Z.GLSZM] == radiomics.unpack_zones(wide.zones.cpu().numpy())["glszm"].tolist()
    again = radiomics.extract(c["scan"], c["mask"], DEV, glszm=True, buffers=wide)          # the buffers are written again
    assert again.zones.data_ptr() == wide.zones.data_ptr() and again.labels.data_ptr() == wide.labels.data_ptr()
    assert again.zones_workspace.data_ptr() == wide.zones_workspace.data_ptr() and all(same(v, alonef[k]) for k, v in radiomics.finish(again, None).items())


# ---- the MLP at the wider tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [98, 228])
def test_mlp_at_zone_width_vs_fp64(width):
    """MLP(width) forward and backward at N = 4, training mode, against the fp64 torch restatement, at the bar tests/test_tail_ops_gpu.py
    holds width 32 to: 98 columns of one modality with all classes and the size zones, 228 = 32 clinical columns + 2 x 98."""
    mlp_at_width(width, MLP_STREAM[width])


# ---- through the Python layer and the command lines ------------------------------------------------------------------------------------------
def test_cli_extraction_tool_with_glszm_writes_the_rows_of_finish(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=13)
    names = radiomics.feature_names("all", glszm=True)
    out = tmp_path / "radiomics.csv"
    log = process(["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--classes", "all", "--glszm",
                    "--out", str(out)], tmp_path)
    assert "196 features" in log
    cols, rows = radiomics.read_csv(out)
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in names] and len(cols) == 1 + 2 * 98 and len(rows) == 3
    for px in ("t1", "t2"):
        ds = ImageDataset(os.path.join(tree["image_loc"], px), tree["key_loc"])
        for p in ds.patients:
            want = radiomics.finish(radiomics.extract(*ds._load(p), DEV, classes="all", glszm=True))
            assert list(want) == list(names) and all(math.isfinite(v) for v in want.values()), p
            row = next(r for r in rows if int(r[0]) == ds._uid_of(p))
            for n, v in want.items():
                assert float(row[cols.index(f"{px}_{n}")]) == v, (p, n)
    # extract_tree itself, the switch alone, in its stacked read-back
    part = radiomics.extract_tree(ImageDataset(os.path.join(tree["image_loc"], "t1"), tree["key_loc"]), DEV, glszm=True)
    assert list(part[0]) == ["MRN"] + list(radiomics.feature_names((), glszm=True)) and len(part[0]) == 64
    assert all(float(rows[k][cols.index("t1_" + n)]) == part[k][n] for k in range(3) for n in radiomics.feature_names((), glszm=True))


def test_cli_trains_the_fusion_model_with_glszm_then_infers(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=14, val_fraction=0.34)
    loc = ["--config", tiny_config(tmp_path, radiomics={"classes": list(radiomics.TEXTURE_CLASSES), "glszm": True}), "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"], "--image_loc", tree["image_loc"]]
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = process([main, "--output_path", str(out), "--radiomics", "--images", "--survival", "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    cols, rows = radiomics.read_csv(out / "radiomics_features.csv")
    assert len(cols) == 1 + 2 * 98 and cols[-1] == "t2_original_glszm_LargeAreaHighGrayLevelEmphasis" and len(rows) == 6
    assert os.path.exists(out / "radiomics_scaler.csv")
    log = process([main, "--output_path", str(out), "--inference", "--radiomics", "--images", "--survival", "--weights",
                    str(out / "best_surv_model.pth"), "--rad_loc", str(out / "radiomics_features.csv"), *loc], out)
    assert "All C-indexes" in log
