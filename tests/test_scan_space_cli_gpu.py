"""`main.py --inference --image_loc DIR --scan_space` as one fresh process on a synthetic patient tree: every class's attention map is
written on the voxel grid of each of the patient's scans, with the scan's geometry, beside the files the inference wrote before.  The
class-0 file must be the restatement (tests/_scan_space_ref.py) of the patient's 64^3 att_map.nii.gz within 2 * 2^-24 * max|map|."""
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd.data import nifti, synth_nifti
from tests import _ingest_ref as R
from tests import _resample_ref as G
from tests import _scan_space_ref as S
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu


def test_cli_writes_every_class_on_every_scan(tmp_path):
    from mmnn_sts_amd.models.densenet import TinyDensenet
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=4, seed=41, val_fraction=0.5)
    # every scan gets a geometry of its own (the tree's is the identity, which a writer that forgot the affine would emit too)
    scans = {}
    for i, uid in enumerate(tree["uids"]):
        for k, mod in enumerate(("t1", "t2")):
            path = os.path.join(tree["image_loc"], mod, f"SYN-{i:04d}-{mod}-a", f"scan_{mod}.nii.gz")
            img = nifti.read(path)
            A = G.affine((("z", 0.05 + 0.01 * i), ("x", -0.03 * (k + 1))), (0.9, 0.8 + 0.1 * k, 3.0), (-40.5 + i, 22.25, -13.0 * (k + 1)))
            nifti.write(path, img.raw, img.slope, img.inter, affine=A)
            mask = nifti.read(os.path.join(os.path.dirname(path), "mask.nii.gz"))
            scans[uid, mod] = (R.read_nifti_file(path), mask.raw)
    torch.manual_seed(5)
    img_model = TinyDensenet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.2)
    weights = tmp_path / "fresh.pth"
    torch.save(MultiModalModel(img_model, [f"predictor{i}" for i in range(32)], 2, 12, blend=False).state_dict(), weights)
    log = run_main(["--inference", "--images", "--preop", "--survival", "--transforms", "--scan_space", "--weights", str(weights),
                    "--config", tiny_config(tmp_path), "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
                    "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]], tmp_path, limit_s=600)
    assert "All C-indexes" in log
    val_uids = [int(l) for l in open(tree["val_uids"]).read().split()]
    assert len(val_uids) == 2
    for i, uid in enumerate(val_uids):
        d = tmp_path / "attention_maps" / f"_patient_{uid}"
        # the files written before: present, in the form they had
        for name in ("t1image", "t2image", "att_map"):
            h = R.read_nifti_file(d / f"{name}.nii.gz")
            assert h["datatype"] == 16 and h["dim"][:4] == (3, 64, 64, 64) and h["data"].dtype == np.float32 and np.isfinite(h["data"]).all()
            assert h["sform_code"] == 2 and np.array_equal(h["srow"], np.eye(4)[:3])
        att = R.read_nifti_file(d / "att_map.nii.gz")["data"]
        assert att.min() >= 0.0 and att.max() <= 1.0 and att.max() > 0.0
        assert np.array_equal(att, np.load(tmp_path / "attention_maps" / f"patient{i}_att_map.npy"))
        assert len(open(d / "preds.txt").read().split()) >= 2
        assert sorted(p.name for p in d.iterdir()) == sorted(["t1image.nii.gz", "t2image.nii.gz", "att_map.nii.gz", "preds.txt"] +
                                                             [f"att_map_class{k}_on_{m}.nii.gz" for k in range(2) for m in ("t1", "t2")])
        for mod in ("t1", "t2"):
            scan, mask_raw = scans[uid, mod]
            keep = S.keep_flags(scan["data"], mask_raw, (scan["scl_slope"], scan["scl_inter"]))
            kept = np.einsum("i,j,k->ijk", *[k.astype(np.int64) for k in keep]).astype(bool)
            assert 0 < kept.sum() < kept.size
            for k in range(2):
                h = R.read_nifti_file(d / f"att_map_class{k}_on_{mod}.nii.gz")
                assert h["datatype"] == 16 and h["data"].dtype == np.float32 and h["dim"][:4] == scan["dim"][:4] and h["dim"][0] == 3
                assert h["sform_code"] == 2 and np.array_equal(h["srow"], scan["srow"]) and not np.array_equal(h["srow"], np.eye(4)[:3])
                data = h["data"]
                assert np.isfinite(data).all() and data.min() >= 0.0 and data.max() <= 1.0
                assert not data[~kept].any()                                                  # zero exactly on every slice the ingest drops
                if k == 0:
                    ref = S.maps_to_scan_ref(att[None], keep)[0]
                    err, tol = float(np.abs(data.astype(np.float64) - ref).max()), S.tolerance(att)
                    print(f"patient {uid}, class 0 on {mod}: scan {data.shape}, max error {err:.3e}, bound {tol:.3e}")
                    assert err <= tol
