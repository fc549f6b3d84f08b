"""`mmnn_radiomics_zones` on the device against the numpy / scipy restatement (tests/_radiomics_zones_ref.py), the size-zone switch through
`radiomics.extract` / `finish` / the command lines, and the MLP at the widths the wider table brings.

The labels, the sizes, the per-level counts and the six integers are compared with array equality.  The 16 fp64 features are held to
tests/_radiomics_zones_cases.py: BOUND relative to the scale the restatement returns beside each value, against the mpmath evaluation of the
same integer tables; the NaN / zero pattern of the flagged cases is exact."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import ingest, synth_nifti
from tests import _radiomics_zones_ref as Z
from tests._radiomics_zones_cases import BOUND, FLAGGED, MLP_STREAM, ZONE_CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 256
PATTERN = 0xA5
_REF = {}


@pytest.fixture(autouse=True)
def _leave_the_dropout_stream_where_it_was():
    """As in tests/test_radiomics_texture_gpu.py: the fused MLP draws from the process-wide seed counter in every forward; tests later in
    the suite were tuned on the masks they get, so the tests of this file put the counter back."""
    from mmnn_sts_amd import ops
    before = ops._seed_counter[0]
    yield
    ops._seed_counter[0] = before


def _ref(name):
    """The restatement of a case and the mpmath evaluation of its tables, computed once and shared."""
    if name not in _REF:
        zn = Z.restate(ZONE_CASES[name])
        zn["exact"] = None if zn["flagged"] else Z.exact(zn)
        _REF[name] = zn
    return _REF[name]


def _device_bytes(arr, lead):
    """(holder, pointer): the array's bytes, x fastest, `lead` bytes past a 256-byte boundary."""
    host = ingest._host_bytes(np.ascontiguousarray(arr))
    buf = torch.zeros(lead + host.size + 64, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[lead:lead + host.size] = torch.from_numpy(host.copy()).to(DEV)
    return buf, buf.data_ptr() + lead


def _run(name):
    """mmnn_radiomics, then mmnn_radiomics_zones through the C-ABI itself: the result block and the three tables sit between guard bytes
    inside one buffer filled with a pattern, and ws3 starts from 0xFF.  Returns dict(block (bytes of the zones block), labels, sizes, levels
    (int64), fields (of the first call))."""
    c = ZONE_CASES[name]
    x, y, z = c["scan"].shape
    mb, n = c["max_bins"], x * y * z
    sizes = [_lib.RADIOMICS_ZONES_BYTES, n * 4, n * 4, mb * 4]
    offs, off = [], GUARD
    for s in sizes:
        offs.append(off)
        off += (s + GUARD + 255) // 256 * 256
    buf = torch.full((off,), PATTERN, dtype=torch.uint8, device=DEV)
    first = torch.full((_lib.RADIOMICS_RESULT_BYTES + mb * 4 + 13 * mb * mb * 4,), PATTERN, dtype=torch.uint8, device=DEV)
    sbuf, sp = _device_bytes(c["scan"], c["scan_lead"])
    mbuf, mp = _device_bytes(c["mask"], c["mask_lead"])
    ws = torch.full((radiomics.workspace_bytes(x, y, z, mb),), 0xFF, dtype=torch.uint8, device=DEV)
    n3 = _lib.lib().mmnn_radiomics_zones_workspace_bytes(x, y, z, mb)
    assert n3 > 0
    ws3 = torch.full((n3,), 0xFF, dtype=torch.uint8, device=DEV)
    desc = _lib.RadiomicsDesc(x, y, z, ingest.TYPE_CODES[c["scan"].dtype], ingest.TYPE_CODES[c["mask"].dtype], *c["scan_scale"], *c["mask_scale"],
                              c["bin_width"], mb)
    stream = torch.cuda.current_stream().cuda_stream
    f, p = first.data_ptr(), buf.data_ptr()
    nb = _lib.RADIOMICS_RESULT_BYTES
    _lib.check(_lib.lib().mmnn_radiomics(ctypes.byref(desc), sp, mp, f, f + nb, f + nb + mb * 4, ws.data_ptr(), stream), "mmnn_radiomics")
    _lib.check(_lib.lib().mmnn_radiomics_zones(ctypes.byref(desc), f, ws.data_ptr(), p + offs[0], p + offs[1], p + offs[2], p + offs[3],
                                               ws3.data_ptr(), stream), "mmnn_radiomics_zones")
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    keep = np.ones(off, dtype=bool)
    for o, s in zip(offs, sizes):
        keep[o:o + s] = False
    assert (b[keep] == PATTERN).all(), f"{name}: bytes outside the zones block and the tables were written"
    cut = [b[o:o + s].copy() for o, s in zip(offs, sizes)]
    return {"block": cut[0], "labels": cut[1].view(np.uint32).astype(np.int64), "sizes": cut[2].view(np.uint32).astype(np.int64),
            "levels": cut[3].view(np.uint32).astype(np.int64), "fields": radiomics.unpack_block(first[:nb].cpu().numpy())}


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
    good = dict(x=4, y=4, z=4, scan_type=4, mask_type=2, scan_slope=1.0, scan_inter=0.0, mask_slope=1.0, mask_inter=0.0, bin_width=25.0, max_bins=16)
    ptrs = [p, p + 65536, p + 1024, p + 2048, p + 4096, p + 8192, p + 32768]      # result, ws, out, labels, sizes, levels, ws3
    for bad in (dict(bin_width=0.0), dict(bin_width=float("nan")), dict(scan_type=3), dict(mask_type=1), dict(x=0), dict(max_bins=0),
                dict(max_bins=_lib.RADIOMICS_MAX_BINS + 1)):
        desc = _lib.RadiomicsDesc(**dict(good, **bad))
        assert L.mmnn_radiomics_zones(ctypes.byref(desc), *ptrs, None) == 1 and _lib.last_error(), bad
    desc = _lib.RadiomicsDesc(**good)
    assert L.mmnn_radiomics_zones(None, *ptrs, None) == 1 and "null" in _lib.last_error()
    for k in range(len(ptrs)):
        assert L.mmnn_radiomics_zones(ctypes.byref(desc), *[None if q == k else v for q, v in enumerate(ptrs)], None) == 1, k      # null
        assert "null" in _lib.last_error()
    for k, step in ((0, 4), (1, 64), (2, 4), (3, 2), (4, 2), (5, 2), (6, 64)):
        assert L.mmnn_radiomics_zones(ctypes.byref(desc), *[v + step if q == k else v for q, v in enumerate(ptrs)], None) == 1, k   # misaligned
        assert "misaligned" in _lib.last_error()
    torch.cuda.synchronize()
    assert not t.any()                                     # refused before any launch: nothing was written


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
    from mmnn_sts_amd.models.mlp import MLP
    from oracle import restatement as OR
    from tests import test_tail_ops_gpu as TT
    from tests._util import synth_sd
    sd = synth_sd(OR.mlp_schema(width, 2, 12), f"radmlp{width}.")
    x, cot = TT._u(f"rad/mlp/x/{width}/{MLP_STREAM[width]}", (4, width)), TT._u(f"rad/mlp/cot/{width}", (4, 12))
    ref, leaves, pres = TT.mlp_ref(sd, x, True)
    TT._assert_off_branch(pres, f"mlp width {width}")
    assert torch.allclose(ref.detach(), OR.mlp_features({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}, x.double(), True, 0.0).detach(),
                          rtol=1e-12, atol=1e-14)
    (ref * cot.double()).sum().backward()
    m = MLP(width, 2, 12, dropout_prob=0.0)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    xg = x.to(DEV).requires_grad_(True)
    f = m.features(m.backbone(xg))
    (f * cot.to(DEV)).sum().backward()
    params = dict(m.named_parameters())
    errs = {"features": TT.rel_err(f.detach().cpu().numpy(), ref.detach().numpy()), "dx": TT.rel_err(xg.grad.cpu().numpy(), leaves["x"].grad.numpy())}
    for k in TT.MLP_PARAM_KEYS:
        errs[k] = TT.mlp_grad_err(k, params[k].grad, leaves, True)
    assert len(errs) == 26
    TT._check(errs, TT.BAR)


# ---- through the Python layer and the command lines ------------------------------------------------------------------------------------------
def _process(argv, cwd):
    env = dict(os.environ, MMNN_POISON_LDS="0", MMNN_POISON_WS="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, *argv], cwd=str(cwd), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def _tiny_config(tmp_path):
    import yaml
    cfg = {"ImageModel": {"name": "tinydensenet", "modality": "t1t2", "feature_layers": 12, "num_classes": 2, "spatial_dims": 3,
                          "in_channels": 2, "dropout_prob": 0.2},
           "ClinicalModel": {"NUM_PREDICTORS": 32, "PRE_OP_PREDICTORS": [], "POST_OP_PREDICTORS": []},
           "Hyperparameters": {"momentum": 0.9, "weight_decay": 1e-4, "train_batch_size": 2, "seed": 42, "class_frequencies": [0.4, 0.55]},
           "Radiomics": {"classes": list(radiomics.TEXTURE_CLASSES), "glszm": True}}
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def test_cli_extraction_tool_with_glszm_writes_the_rows_of_finish(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=13)
    names = radiomics.feature_names("all", glszm=True)
    out = tmp_path / "radiomics.csv"
    log = _process(["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--classes", "all", "--glszm",
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
    loc = ["--config", _tiny_config(tmp_path), "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"], "--image_loc", tree["image_loc"]]
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = _process([main, "--output_path", str(out), "--radiomics", "--images", "--survival", "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    cols, rows = radiomics.read_csv(out / "radiomics_features.csv")
    assert len(cols) == 1 + 2 * 98 and cols[-1] == "t2_original_glszm_LargeAreaHighGrayLevelEmphasis" and len(rows) == 6
    assert os.path.exists(out / "radiomics_scaler.csv")
    log = _process([main, "--output_path", str(out), "--inference", "--radiomics", "--images", "--survival", "--weights",
                    str(out / "best_surv_model.pth"), "--rad_loc", str(out / "radiomics_features.csv"), *loc], out)
    assert "All C-indexes" in log
