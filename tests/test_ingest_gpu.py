"""The device ingest (csrc/ingest.hip, mmnn_sts_amd/data/ingest.py) against the fp64 restatement of tests/_ingest_ref.py, the collate
function built on it, and `main.py --image_loc` as a fresh process on a synthetic patient tree.

Parity bound: the extents are equal EXACTLY; the plane is within 2 * 2^-24 * max|v| absolute (max over the finite voxels of the masked
volume).  Derivation: v and the window sums are fp64 on both sides, so the only visible error is the final rounding of a mean whose
magnitude is at most max|v| -- half a unit of 2^-24 max|v|; summation order in fp64 adds ~1e-16 relative; two units are allowed."""
import functools
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd.data import ingest, nifti, synth_nifti
from tests import _ingest_ref as R
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (97, 130, 23)
SENTINEL = 1.0e30          # no plane can hold it: the voxels are below 2^15


def _run_ingest(scan, mask, ss=(1.0, 0.0), ms=(1.0, 0.0)):
    out = torch.full((64, 64, 64), float("nan"), device=DEV)
    ext = ingest.ingest_volume(ingest.upload(scan, DEV, *ss), ingest.upload(mask, DEV, *ms), out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tuple(ext.cpu().tolist())


def _check(scan, mask, ss=(1.0, 0.0), ms=(1.0, 0.0), label=""):
    ref, ext_ref, v = R.ingest_ref(scan, mask, ss, ms)
    got, ext = _run_ingest(scan, mask, ss, ms)
    tol = R.tolerance(v)
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    ok = ~nan_ref & ~nan_got
    err = float(np.abs(got[ok].astype(np.float64) - ref[ok]).max()) if ok.any() else 0.0
    print(f"{label}: extents {ext} (ref {ext_ref}), max error {err:.3e}, bound {tol:.3e} ({err / tol if tol else 0.0:.2f} of it), "
          f"NaN windows {int(nan_got.sum())} (ref {int(nan_ref.sum())})")
    assert ext == ext_ref
    assert np.array_equal(nan_got, nan_ref)
    assert err <= tol
    return got, ext


def _holey_mask(shape, dtype="u1", value=1):
    """A box well inside the volume with interior empty slices on all three axes."""
    lo = tuple(max(1, n // 8) for n in shape)
    hi = tuple(n - max(2, n // 6) for n in shape)
    holes = tuple((lo[a] + 2, lo[a] + 3, hi[a] - 3) for a in range(3))
    return R.box_mask(shape, lo, hi, holes, dtype, value)


@pytest.mark.parametrize("code", sorted(R.NP_OF_CODE))
def test_parity_every_scan_type(code):
    rng = np.random.default_rng(100 + code)
    _check(R.random_scan(rng, SHAPE, code), _holey_mask(SHAPE), label=f"scan type {code}")


@pytest.mark.parametrize("mask_dtype", ["u1", "i2", "f4", "f4-soft"])
def test_parity_mask_types(mask_dtype):
    rng = np.random.default_rng(7)
    scan = R.random_scan(rng, SHAPE, 4)
    if mask_dtype == "f4-soft":                       # a non-binary float mask: weights in (0, 1] inside the box
        mask = _holey_mask(SHAPE, "f4") * (0.25 + 0.75 * rng.random(SHAPE)).astype(np.float32)
    else:
        mask = _holey_mask(SHAPE, mask_dtype, 1 if mask_dtype != "i2" else 3)
    _check(scan, mask, label=f"mask {mask_dtype}")


def test_parity_replication_on_one_axis_and_faces():
    rng = np.random.default_rng(8)
    shape = (150, 140, 40)
    scan = R.random_scan(rng, shape, 16)
    _, ext = _check(scan, _holey_mask(shape), label="z below 64, x / y above")
    assert ext[2] < 64 < min(ext[:2])
    mask = R.box_mask(shape, (0, 0, 0), (150, 90, 40), holes=((70,), (40, 41), (17,)))      # the box touches five faces
    _, ext = _check(scan, mask, label="box on the faces")
    assert ext == (149, 88, 39)


def test_parity_full_mask_nothing_removed():
    rng = np.random.default_rng(9)
    shape = (256, 256, 40)
    scan = R.random_scan(rng, shape, 4)
    _, ext = _check(scan, np.ones(shape, dtype=np.uint8), label="full mask 256x256x40")
    assert ext == shape


def test_parity_nan_voxel_keeps_its_slice():
    rng = np.random.default_rng(10)
    scan = R.random_scan(rng, SHAPE, 16)
    mask = _holey_mask(SHAPE)
    hole_x = max(1, SHAPE[0] // 8) + 2
    assert not mask[hole_x].any()
    _, ext0 = _check(scan, mask, label="before the NaN")
    scan[hole_x, 60, 11] = np.nan                    # NaN * 0 = NaN: the otherwise empty slice x = hole_x is kept
    got, ext = _check(scan, mask, label="one NaN voxel")
    assert ext == (ext0[0] + 1, ext0[1], ext0[2]) and 0 < np.isnan(got).sum() < 64


def test_parity_slope_inter_background_and_exact_zeros():
    rng = np.random.default_rng(11)
    # an inter that makes the background non-zero everywhere: only the mask decides
    scan = R.random_scan(rng, SHAPE, 4)
    _, ext = _check(scan, _holey_mask(SHAPE), ss=(0.5, 50.25), label="int16, slope 0.5, inter 50.25")
    assert ext == R.ingest_ref(scan, _holey_mask(SHAPE))[1]
    # masked voxels that are exactly zero after raw * slope + inter (rounded multiply, rounded add -- a fused multiply-add would leave
    # a residue on them): slice x = k of a float64 scan is such voxels only, so it counts as empty although the mask covers it
    slope = np.float32(0.3)
    inter, raws = R.exact_zero_raws(slope)
    scan = R.random_scan(rng, SHAPE, 64) + 1000.0
    mask = _holey_mask(SHAPE)
    k = SHAPE[0] // 2
    assert mask[k].any()
    scan[k] = rng.choice(raws, size=SHAPE[1:])
    _, ext_plain = _check(R.random_scan(rng, SHAPE, 64) + 1000.0, mask, ss=(slope, inter), label="float64 scaled, no zero slice")
    _, ext = _check(scan, mask, ss=(slope, inter), label="float64 scaled, slice of exact zeros")
    assert ext == (ext_plain[0] - 1, ext_plain[1], ext_plain[2])
    # the mask's own slope / inter, and a degenerate slope (= unscaled)
    _check(R.random_scan(rng, SHAPE, 512), _holey_mask(SHAPE, "i2", 4), ss=(float("nan"), 9.0), ms=(0.25, 0.0), label="mask scaled, scan slope NaN")


def test_empty_mask_gives_zeros_and_zero_extents():
    rng = np.random.default_rng(12)
    got, ext = _check(R.random_scan(rng, SHAPE, 4), np.zeros(SHAPE, dtype=np.uint8), ss=(2.0, 1.0), label="all-zero mask")
    assert ext == (0, 0, 0) and not got.any()


def test_parity_512x512x48_once():
    rng = np.random.default_rng(13)
    shape = (512, 512, 48)
    scan = rng.integers(1, 3000, shape, dtype=np.int16)
    mask = R.box_mask(shape, (96, 101, 4), (416, 411, 43))
    _, ext = _check(scan, mask, ss=(0.25, -12.5), label="512x512x48 int16, 320x310x39 box")
    assert ext == (320, 310, 39)


def test_plane_lands_in_its_channel_only_and_repeats_bitwise():
    rng = np.random.default_rng(14)
    scan, mask = R.random_scan(rng, SHAPE, 4), _holey_mask(SHAPE)
    batch = torch.full((2, 2, 64, 64, 64), SENTINEL, device=DEV)
    s, m = ingest.upload(scan, DEV, 0.5, 3.0), ingest.upload(mask, DEV)
    ingest.ingest_volume(s, m, batch[1, 0])
    again = torch.empty((64, 64, 64), device=DEV)
    ingest.ingest_volume(s, m, again)
    torch.cuda.synchronize()
    b = batch.cpu()
    assert (b[0] == SENTINEL).all() and (b[1, 1] == SENTINEL).all() and not (b[1, 0] == SENTINEL).any()
    assert torch.equal(b[1, 0], again.cpu())
    ref, _, v = R.ingest_ref(scan, mask, (0.5, 3.0))
    assert np.abs(b[1, 0].double().numpy() - ref).max() <= R.tolerance(v)
    with pytest.raises(ValueError):
        ingest.ingest_volume(s, m, batch[:, 0, 0])                                         # not a 64^3 plane
    with pytest.raises(ValueError):
        ingest.ingest_volume(s, ingest.upload(mask[:-1], DEV), again)                      # extents differ


def test_big_endian_file_ingests_like_its_twin(tmp_path):
    rng = np.random.default_rng(15)
    scan, mask = R.random_scan(rng, (40, 36, 20), 4), _holey_mask((40, 36, 20))
    planes = []
    for bo in "<>":
        (tmp_path / f"scan{bo == '<'}.nii").write_bytes(R.pack_nifti(scan, 4, 0.5, -2.0, bo))
        (tmp_path / f"mask{bo == '<'}.nii").write_bytes(R.pack_nifti(mask, 2, byteorder=bo))
        out = torch.empty((64, 64, 64), device=DEV)
        ingest.ingest_volume(nifti.read(tmp_path / f"scan{bo == '<'}.nii"), nifti.read(tmp_path / f"mask{bo == '<'}.nii"), out)
        planes.append(out.cpu())
    assert torch.equal(planes[0], planes[1])
    ref, _, v = R.ingest_ref(scan, mask, (0.5, -2.0))
    assert np.abs(planes[0].double().numpy() - ref).max() <= R.tolerance(v)


# ---- collate ----------------------------------------------------------------------------------------------------------------------
def test_collate_equals_the_single_volume_results_and_feeds_val_transforms(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    from mmnn_sts_amd.transforms import val_transforms
    tree = synth_nifti.write_tree(tmp_path, n_patients=2, seed=21)
    ds = T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])
    coll = ingest.IngestCollate(DEV)
    x, ev, du = coll([ds[0], ds[1]])
    assert x.shape == (2, 2, 64, 64, 64) and x.dtype == torch.float32 and x.is_cuda and ev.shape == du.shape == (2, 2)
    uids, ext = coll.pending[0]
    assert uids == ds.uids and ext.shape == (2, 2, 3) and ext.dtype == torch.int32
    ref = np.zeros((2, 2, 64, 64, 64))
    for n in range(2):
        for c, (scan, mask) in enumerate(ds[n][0].volumes):
            single = torch.empty((64, 64, 64), device=DEV)
            e = ingest.ingest_volume(scan, mask, single)
            assert torch.equal(single, x[n, c]) and torch.equal(e, ext[n, c])                # bit for bit
            ref[n, c], e_ref, _ = R.ingest_ref(scan.raw, mask.raw, (scan.slope, scan.inter), (mask.slope, mask.inter))
            assert tuple(e.tolist()) == e_ref
    assert coll.take_empty() == [] and coll.pending == []
    a = val_transforms(x)
    b = val_transforms(torch.from_numpy(ref).float().to(DEV))
    err = float((a - b).abs().max())
    print(f"val_transforms of the collated batch vs of the restatement: max abs difference {err:.3e}")
    assert err <= 1e-5


# ---- main.py --image_loc, fresh processes, one at a time ---------------------------------------------------------------------------
_main = functools.partial(run_main, limit_s=900)


def _loc(tree):
    return ["--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
            "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]


def test_cli_fusion_training_then_inference_with_nifti_export(tmp_path):
    from mmnn_sts_amd.models.densenet import TinyDensenet
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=31)
    cfg = tiny_config(tmp_path)
    log = _main(["--images", "--preop", "--survival", "--blend", "--transforms", "--epochs", "1", "--config", cfg, *_loc(tree)], tmp_path)
    assert "epoch 1/1" in log
    img = TinyDensenet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.2)
    MultiModalModel(img, [f"p{i}" for i in range(32)], 2, 12, blend=True).load_state_dict(torch.load(tmp_path / "best_surv_model.pth"), strict=True)
    log = _main(["--inference", "--images", "--preop", "--survival", "--transforms", "--weights", str(tmp_path / "best_surv_model.pth"),
                 "--config", cfg, *_loc(tree)], tmp_path)
    assert "All C-indexes" in log
    val_uids = [int(l) for l in open(tree["val_uids"]).read().split()]
    assert len(val_uids) >= 2
    for i, uid in enumerate(val_uids):
        d = tmp_path / "attention_maps" / f"_patient_{uid}"
        for name in ("t1image", "t2image", "att_map"):
            h = R.read_nifti_file(d / f"{name}.nii.gz")
            assert h["datatype"] == 16 and h["dim"][:4] == (3, 64, 64, 64) and h["data"].dtype == np.float32 and np.isfinite(h["data"]).all()
        att = R.read_nifti_file(d / "att_map.nii.gz")["data"]
        assert att.min() >= 0.0 and att.max() <= 1.0
        assert np.array_equal(att, np.load(tmp_path / "attention_maps" / f"patient{i}_att_map.npy"))      # the .npy files stay as they are
        preds = [float(l) for l in open(d / "preds.txt").read().split()]
        assert len(preds) >= 2 and np.isfinite(preds).all()


def test_cli_unimodal_classification_one_epoch(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=32)
    log = _main(["--images", "--classification", "--epochs", "1", "--config", tiny_config(tmp_path, "t1", 1), *_loc(tree)], tmp_path)
    assert "epoch 1/1" in log and os.path.exists(tmp_path / "final_model.pth")


def test_cli_empty_mask_is_reported_by_uid(tmp_path):
    bad = 1000 + 7 * 2
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=33, empty_mask_uids=(bad,))
    r = _main(["--images", "--survival", "--epochs", "2", "--config", tiny_config(tmp_path, "t2", 1), *_loc(tree)], tmp_path, expect_ok=False)
    log = r.stdout + r.stderr
    assert r.returncode != 0, log[-2000:]
    assert f"{bad}" in log and "empty mask" in log
    assert "epoch 1/2" in log and "epoch 2/2" not in log                                    # the run ends with the epoch that met it
