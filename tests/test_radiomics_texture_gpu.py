"""`mmnn_radiomics_texture` on the device against the numpy restatement (tests/_radiomics_texture_ref.py), the texture classes through
`radiomics.extract` / `finish` / the command lines, and the MLP at the widths the wider table brings.

The four integer tables (run-length, dependence, NGTDM counts and sums) are compared with array equality.  The 35 fp64 features are held to
tests/_radiomics_texture_cases.py: BOUND relative to the scale the restatement returns beside each value, against the mpmath evaluation of
the same tables; NaN patterns and the NGTDM's special values (10^6, 0) are exact."""
import math
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import synth_nifti
from tests import _radiomics_texture_ref as T
from tests._radiomics_harness import (DEV, ROOT, cut, first_call, follow_call, leave_the_dropout_stream_where_it_was, mlp_at_width,  # noqa: F401
                                      process, refusal_walk)
from tests._cli import tiny_config
from tests._radiomics_texture_cases import BOUND, FLAGGED, MLP_STREAM, TEXTURE_CASES

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(name):
    """The restatement of a case and the mpmath evaluation of its tables, computed once and shared."""
    if name not in _REF:
        tex = T.restate(TEXTURE_CASES[name])
        tex["exact"] = None if tex["flagged"] else T.exact(tex)
        _REF[name] = tex
    return _REF[name]


def _run(name):
    """mmnn_radiomics, then mmnn_radiomics_texture through the C-ABI itself: the texture block and the four tables sit between guard
    bytes inside one buffer filled with a pattern.  Returns dict(block (bytes of the texture block), glrlm, gldm, ngtdm_n, ngtdm_s (int64),
    fields (of the first call), first (the first call's result block, hist and glcm, as bytes))."""
    c = TEXTURE_CASES[name]
    mb, L = c["max_bins"], max(c["scan"].shape)
    sizes = [_lib.RADIOMICS_TEXTURE_BYTES, 13 * mb * L * 4, mb * 27 * 4, mb * 27 * 4, mb * 27 * 8]
    r, desc, first, _, _ = first_call(c)
    buf, offs, _, _ = follow_call(r, desc, "texture", sizes)
    torch.cuda.synchronize()
    got = cut(buf, offs, sizes, f"{name}: bytes outside the texture block and the tables were written")
    return {"block": got[0], "glrlm": got[1].view(np.uint32).astype(np.int64).reshape(13, mb, L),
            "gldm": got[2].view(np.uint32).astype(np.int64).reshape(mb, 27), "ngtdm_n": got[3].view(np.uint32).astype(np.int64).reshape(mb, 27),
            "ngtdm_s": got[4].view(np.uint64).astype(np.int64).reshape(mb, 27),
            "fields": radiomics.unpack_block(first[:_lib.RADIOMICS_RESULT_BYTES].cpu().numpy()), "first": first.cpu().numpy()}


@pytest.mark.parametrize("name", list(TEXTURE_CASES))
def test_against_restatement(name):
    tex, got = _ref(name), _run(name)
    ref = tex["ref"]
    assert (got["fields"]["empty"], got["fields"]["nonfinite"], got["fields"]["overflow"]) == (ref["empty"], ref["nonfinite"], ref["overflow"])
    for k in ("glrlm", "gldm", "ngtdm_n", "ngtdm_s"):
        assert np.array_equal(got[k], tex[k]), (name, k, int(np.abs(got[k] - tex[k]).sum()))
    dev_f = radiomics.unpack_texture(got["block"])
    if name in FLAGGED:
        assert tex["flagged"] and all(np.isnan(dev_f[c]).all() for c in dev_f) and not any(got[k].any() for k in ("glrlm", "gldm", "ngtdm_n", "ngtdm_s"))
        return
    values = {"glrlm": dict(zip(T.GLRLM, dev_f["glrlm"])), "gldm": dict(zip(T.GLDM, dev_f["gldm"])), "ngtdm": dict(zip(T.NGTDM, dev_f["ngtdm"]))}
    for cls, feats in tex["features"].items():
        for k, (want, _) in feats.items():
            assert math.isnan(want) == math.isnan(values[cls][k]), (name, cls, k, values[cls][k], want)
            if cls == "ngtdm" and want in (0.0, 1.0e6):
                assert values[cls][k] == want, (name, k, values[cls][k], want)          # the special values are exact
    own = T.deviations(tex, {cls: {k: v[0] for k, v in f.items()} for cls, f in tex["features"].items()}, tex["exact"])
    dev = T.deviations(tex, values, tex["exact"])
    print(name, "restatement", {k: f"{v / 2 ** -53:.2f}" for k, v in own.items()}, "device", {k: f"{v / 2 ** -53:.2f}" for k, v in dev.items()})
    for cls in T.CLASSES:
        assert dev[cls] <= BOUND[cls], (name, cls, "device", dev[cls] / 2 ** -53, values, tex["features"])
    if name == "single_voxel":
        assert np.isnan(dev_f["ngtdm"]).all() and np.isfinite(dev_f["glrlm"]).all() and np.isfinite(dev_f["gldm"]).all()
    if name == "constant":
        assert dev_f["ngtdm"].tolist() == [1.0e6, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("name", ["ellipsoid", "run_ng256_l64", "run_ng300_l64", "nbhd_ng128", "nbhd_ng129", "long_row"])
def test_two_calls_agree_bit_for_bit(name):
    a, b = _run(name), _run(name)
    for k in ("block", "glrlm", "gldm", "ngtdm_n", "ngtdm_s"):
        assert np.array_equal(a[k], b[k]), (name, k)


def test_refusals():
    L = _lib.lib()
    assert L.mmnn_radiomics_texture_workspace_bytes(0, 4, 4, 256) == -1 and L.mmnn_radiomics_texture_workspace_bytes(4, 4, -1, 256) == -1
    assert L.mmnn_radiomics_texture_workspace_bytes(4, 4, 4, 0) == -1
    assert L.mmnn_radiomics_texture_workspace_bytes(4, 4, 4, _lib.RADIOMICS_MAX_BINS + 1) == -1
    assert L.mmnn_radiomics_texture_workspace_bytes(2048, 2048, 512, 256) == -1          # 2^31 voxels
    t = torch.zeros(1 << 17, dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    ptrs = [p, p + 65536, p + 1024, p + 2048, p + 8192, p + 12288, p + 16384, p + 32768]      # result, ws, out, glrlm, gldm, n, s, ws2
    refusal_walk(lambda desc, q: L.mmnn_radiomics_texture(desc, *q, None), ptrs,
                 ((0, 4), (1, 64), (2, 4), (3, 2), (4, 2), (5, 2), (6, 4), (7, 64)),
                 (dict(bin_width=0.0), dict(bin_width=float("nan")), dict(scan_type=3), dict(mask_type=1), dict(x=0), dict(max_bins=0),
                  dict(max_bins=_lib.RADIOMICS_MAX_BINS + 1)), t)


def test_without_classes_the_extraction_is_what_it_was():
    c = TEXTURE_CASES["seven_levels"]                       # (no header scaling, no lead: `extract` on the arrays sees what `_run` uploads)
    plain = radiomics.extract(c["scan"], c["mask"], DEV)
    same = radiomics.extract(c["scan"], c["mask"], DEV, classes=())
    tex = radiomics.extract(c["scan"], c["mask"], DEV, classes=radiomics.TEXTURE_CLASSES)
    assert plain.texture is None and plain.glrlm is None and plain.texture_workspace is None and plain.classes == () and same.texture is None
    feats = radiomics.finish(plain, None)
    assert list(feats) == list(radiomics.FEATURE_NAMES) and len(feats) == 47
    # the block, hist and glcm of the C call itself, which the texture call leaves alone
    first = _run("seven_levels")["first"]
    nb, mb = _lib.RADIOMICS_RESULT_BYTES, c["max_bins"]
    block, hist = first[:nb], first[nb:nb + mb * 4].view(np.uint32).astype(np.int64)
    glcm = first[nb + mb * 4:].view(np.uint32).astype(np.int64).reshape(13, mb, mb)
    for r in (plain, same, tex):
        assert np.array_equal(r.block.cpu().numpy(), block)
        assert np.array_equal(r.hist.cpu().numpy().astype(np.int64), hist) and np.array_equal(r.glcm.cpu().numpy().astype(np.int64), glcm)
    wide = radiomics.finish(tex, None)
    assert list(wide) == list(radiomics.feature_names(radiomics.TEXTURE_CLASSES)) and all(wide[k] == v or (math.isnan(v) and math.isnan(wide[k])) for k, v in feats.items())
    only = radiomics.finish(radiomics.extract(c["scan"], c["mask"], DEV, classes=["ngtdm"], buffers=tex), None)
    assert list(only) == list(radiomics.feature_names(["ngtdm"])) and all(only[k] == wide[k] for k in only)


# ---- the MLP at the wider tables -----------------------------------------------------------------------------------------------------------
# input stream per width: tests/_radiomics_texture_cases.py: MLP_STREAM states the rule


@pytest.mark.parametrize("width", [82, 164, 196])
def test_mlp_at_texture_width_vs_fp64(width):
    """tests/_radiomics_harness.py: mlp_at_width: 82 columns of one modality with all classes, 164 of two, 196 with the 32 clinical columns
    in front."""
    mlp_at_width(width, MLP_STREAM[width])


# ---- through the Python layer and the command lines ------------------------------------------------------------------------------------------
def test_cli_extraction_tool_with_all_classes_writes_the_rows_of_finish(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=11)
    names = radiomics.feature_names(radiomics.TEXTURE_CLASSES)
    out = tmp_path / "radiomics.csv"
    log = process(["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--classes", "all", "--out", str(out)],
                   tmp_path)
    assert "164 features" in log
    cols, rows = radiomics.read_csv(out)
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in names] and len(cols) == 1 + 2 * 82 and len(rows) == 3
    for px in ("t1", "t2"):
        ds = ImageDataset(os.path.join(tree["image_loc"], px), tree["key_loc"])
        for p in ds.patients:
            want = radiomics.finish(radiomics.extract(*ds._load(p), DEV, classes=radiomics.TEXTURE_CLASSES))
            assert list(want) == list(names) and all(math.isfinite(v) for v in want.values()), p
            row = next(r for r in rows if int(r[0]) == ds._uid_of(p))
            for n, v in want.items():
                assert float(row[cols.index(f"{px}_{n}")]) == v, (p, n)
    # extract_tree itself, one class, in its stacked read-back
    part = radiomics.extract_tree(ImageDataset(os.path.join(tree["image_loc"], "t1"), tree["key_loc"]), DEV, classes=["gldm"])
    assert list(part[0]) == ["MRN"] + list(radiomics.feature_names(["gldm"])) and len(part[0]) == 62
    assert all(float(rows[k][cols.index("t1_" + n)]) == part[k][n] for k in range(3) for n in radiomics.feature_names(["gldm"]))


def test_cli_trains_the_fusion_model_on_the_wider_table_then_infers(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=12, val_fraction=0.34)
    loc = ["--config", tiny_config(tmp_path, radiomics={"classes": list(radiomics.TEXTURE_CLASSES)}), "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"], "--image_loc", tree["image_loc"]]
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = process([main, "--output_path", str(out), "--radiomics", "--images", "--survival", "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    cols, rows = radiomics.read_csv(out / "radiomics_features.csv")
    assert len(cols) == 1 + 2 * 82 and cols[-1] == "t2_original_ngtdm_Strength" and len(rows) == 6
    log = process([main, "--output_path", str(out), "--inference", "--radiomics", "--images", "--survival", "--weights",
                    str(out / "best_surv_model.pth"), "--rad_loc", str(out / "radiomics_features.csv"), *loc], out)
    assert "All C-indexes" in log
