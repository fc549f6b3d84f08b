"""The two paths behind the margin step.  Image path: a tree ingested with `mask_margin_mm=r` gives, bit for bit, the batch and extents of
the same tree whose masks were dilated on the host by the restatement (tests/_mask_margin_ref.py) and written as 0 / 1 -- from NIfTI
files, through the DICOM twins with a mask series, an RTSTRUCT and a SEG file, at two plane sizes, and out of the volume cache on the
second pass; `maps_to_scan` lays a map back on the widened box.  Radiomics path: the `shell-<r>-mm_*` columns are those of an extraction
under the restated shell mask, the `original_*` ones those of a run without shells.  And the command lines, one fresh process each."""
import os
import shutil

import numpy as np
import pytest
import torch

from mmnn_sts_amd import radiomics
from mmnn_sts_amd.data import cache as C
from mmnn_sts_amd.data import ingest, nifti, synth_dicom, synth_nifti
from mmnn_sts_amd.data.ImageDatasets import ImageDataset, ImageDatasetByUIDs, T1T2SurvivalDataset
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _mask_margin_ref as M
from tests import _scan_space_ref as S
from tests._radiomics_harness import ROOT, leave_the_dropout_stream_where_it_was, process  # noqa: F401  (the fixture is autouse)
from tests._cli import tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADIUS = 3.3                                 # mm: 3 to 4 voxels in plane and one slice at the trees' spacing (0.9, 0.8 / 0.9, 3.0)


def _dataset(tree, **kw):
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"], **kw)


def _tree(root, n, seed, **kw):
    """A NIfTI tree whose scans and masks share a geometry of their own (rotated, 0.9 x 0.8 / 0.9 x 3.0 mm)."""
    from tests.test_rtstruct_gpu import _with_geometry
    tree = synth_nifti.write_tree(root, n_patients=n, seed=seed, **kw)
    _with_geometry(tree, n)
    return tree


def _dilated_on_the_host(tree, root, radius):
    """The twin of `tree` under `root` whose masks are the restatement's dilation by `radius` mm, written as uint8 0 / 1."""
    shutil.copytree(os.path.dirname(tree["image_loc"]), root)
    twin = {k: (v.replace(os.path.dirname(tree["image_loc"]), str(root)) if isinstance(v, str) else v) for k, v in tree.items()}
    grew = 0
    for mod in ("t1", "t2"):
        for patient in sorted(os.listdir(os.path.join(twin["image_loc"], mod))):
            path = os.path.join(twin["image_loc"], mod, patient, "mask.nii.gz")
            mask = nifti.read(path)
            wide = M.margin(mask.raw, radiomics.spacing_of(mask.affine), radius, "dilate", mask.slope, mask.inter)[0]
            grew += int(wide.sum()) - int((mask.raw != 0).sum())
            nifti.write(path, wide, affine=mask.affine)
    assert grew > 0
    return twin


def _batch(ds, n, **kw):
    x, e = ingest.collate_volumes([ds[i][0].volumes for i in range(n)], DEV, **kw)
    torch.cuda.synchronize()
    return x, e


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("margin")
    plain = _tree(root / "nifti", 4, 21, val_fraction=0.5)
    return plain, _dilated_on_the_host(plain, root / "wide", RADIUS)


@pytest.mark.parametrize("size", [64, 24])
def test_margin_ingest_equals_the_ingest_of_host_dilated_masks(trees, size):
    plain, wide = trees
    x_w, e_w = _batch(_dataset(wide), 4, size=size)
    x_m, e_m = _batch(_dataset(plain), 4, size=size, mask_margin_mm=RADIUS)
    x_p, e_p = _batch(_dataset(plain), 4, size=size)
    assert x_m.shape == (4, 2, size, size, size) and torch.equal(e_m, e_w) and torch.equal(x_m, x_w), int((x_m != x_w).sum())
    assert bool((e_m >= e_p).all()) and bool((e_m > e_p).any()) and not torch.equal(x_m, x_p)       # the rim's slices are kept
    # absent and None are the call it always was
    x_n, e_n = _batch(_dataset(plain), 4, size=size, mask_margin_mm=None)
    assert torch.equal(x_n, x_p) and torch.equal(e_n, e_p)


def test_a_mask_of_255_no_longer_scales_the_plane(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "t", n_patients=1, seed=3)
    ds = ImageDataset(os.path.join(tree["image_loc"], "t1"), tree["key_loc"])
    scan, mask = ds._load(ds.patients[0])
    loud = (mask.raw != 0).astype(np.uint8) * 255
    plane = lambda m, **kw: ingest.collate_volumes([[(scan, m)]], DEV, size=16, **kw)[0]
    a, b = plane(loud, mask_margin_mm=2.0), plane((mask.raw != 0).astype(np.uint8), mask_margin_mm=2.0)
    assert torch.equal(a, b) and float(a.abs().max()) > 0.0
    assert not torch.equal(plane(loud), plane((mask.raw != 0).astype(np.uint8)))                   # without the margin it does


@pytest.mark.parametrize("mask_format", ["series", "rtstruct", "seg"])
def test_dicom_twins_with_a_margin_equal_the_host_dilated_nifti_tree(trees, tmp_path, mask_format):
    plain, wide = trees
    dtree = synth_dicom.from_nifti_tree(os.path.dirname(plain["image_loc"]), tmp_path / "dicom", seed=21, mask_format=mask_format)
    d, w = _dataset(dtree), _dataset(wide)
    assert d.layout == "dicom" and d.uids == w.uids
    # on the restatement alone: under the spacing the DICOM geometry gives, the dilation is the one the wide tree holds
    p = _dataset(plain)
    for i in range(4):
        for (s, _), (_, wm), (_, pm) in zip(d[i][0].volumes, w[i][0].volumes, p[i][0].volumes):
            assert np.array_equal(M.margin(pm.raw, radiomics.spacing_of(s.affine), RADIUS)[0], wm.raw)
    x_d, e_d = _batch(d, 4, mask_margin_mm=RADIUS)
    x_w, e_w = _batch(w, 4)
    assert torch.equal(e_d, e_w) and torch.equal(x_d, x_w), int((x_d != x_w).sum())
    assert int(e_d.min()) > 0 and float(x_d.abs().max()) > 0.0


def test_the_cache_stores_what_the_margin_ingest_made(trees, monkeypatch):
    plain, wide = trees
    want = ingest.IngestCollate(DEV, size=8)
    ref = ImageDatasetByUIDs(_dataset(wide), _dataset(wide).uids)
    batches = [[0, 1], [2, 3]]
    wanted = {tuple(b): (want([ref[i] for i in b])[0], want.pending[-1][1]) for b in batches}
    ds = _dataset(plain)
    cache = C.VolumeCache(DEV, 2, 8, 4)
    collate = ingest.IngestCollate(DEV, size=8, cache=cache, mask_margin_mm=RADIUS)
    sub = C.CachedByUIDs(ds, ds.uids, cache)
    for epoch in range(2):
        if epoch == 1:
            def refuse(*a, **k):
                raise AssertionError("a file was read for a patient the cache holds")
            monkeypatch.setattr(nifti, "read", refuse)
        for b in batches if epoch == 0 else [[3, 0], [1, 2]]:
            x, _, _ = collate([sub[i] for i in b])
            e = collate.pending[-1][1]
            torch.cuda.synchronize()
            for k, i in enumerate(b):
                src = next(bb for bb in batches if i in bb)
                assert torch.equal(x[k], wanted[tuple(src)][0][src.index(i)]) and torch.equal(e[k], wanted[tuple(src)][1][src.index(i)]), (epoch, i)
    assert cache.table.take_counters() == (4, 4, 0)


def test_maps_come_back_on_the_widened_box(trees):
    plain, _ = trees
    ds = _dataset(plain)
    collate = ingest.IngestCollate(DEV, keep_workspaces=True, size=16, mask_margin_mm=RADIUS)
    collate([ds[0]])
    torch.cuda.synchronize()
    ones = torch.ones((1, 16, 16, 16), device=DEV)
    widened = 0
    for c, (scan, mask) in enumerate(ds[0][0].volumes):
        kv = collate.last_volumes[0][c]
        assert kv.shape == scan.shape
        back = ingest.maps_to_scan(ones, kv.shape, kv.workspace)[0].permute(2, 1, 0).cpu().numpy()
        wide = M.margin(mask.raw, radiomics.spacing_of(scan.affine), RADIUS)[0]
        kx, ky, kz = S.keep_flags(scan.raw, wide, (scan.slope, scan.inter))
        box = kx[:, None, None] & ky[None, :, None] & kz[None, None, :]
        assert np.array_equal(back != 0.0, box), f"channel {c}"
        narrow = S.keep_flags(scan.raw, mask.raw, (scan.slope, scan.inter), (mask.slope, mask.inter))
        widened += int(box.sum()) - int((narrow[0][:, None, None] & narrow[1][None, :, None] & narrow[2][None, None, :]).sum())
    assert widened > 0


# ---- the radiomics path ------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def _pair(seed=4, shape=(30, 26, 12), spacing=(0.8, 0.9, 3.0)):
    rng = np.random.default_rng(seed)
    scan = rng.integers(0, 900, shape).astype(np.int16)
    mask = synth_nifti.ellipsoid_mask(shape, rng)
    dev = ingest.upload(scan, torch.device(DEV))
    dev.affine = np.diag([*spacing, 1.0])
    return dev, mask, spacing


def test_shell_columns_are_those_of_an_extraction_under_the_restated_shell():
    scan, mask, spacing = _pair()
    kw = dict(classes="all", glszm=True, mesh=True, bin_width=25.0)
    plain = radiomics.extract(scan, mask, DEV, **kw)
    res = radiomics.extract(scan, mask, DEV, shell_mm=[5, 2.5], **kw)
    assert plain.shell == () and plain.shell_workspace is None and [r for r, _ in res.shell] == [2.5, 5.0]
    want, feats = radiomics.finish(plain), radiomics.finish(res)
    names = radiomics.feature_names("all", True, True, shell_mm=(2.5, 5))
    assert list(feats) == list(names) and list(feats)[:len(want)] == list(want)
    for k, v in want.items():                                                      # the original image's columns: byte for byte
        assert np.array_equal(_bits(feats[k]), _bits(v)), k
    for k in ("block", "hist", "glcm", "texture", "zones", "mesh"):
        assert torch.equal(getattr(plain, k), getattr(res, k)), k
    for r, sub in res.shell:
        rim = M.margin(mask, spacing, r, "shell")[0]
        assert 0 < rim.sum() and not (rim & (mask != 0)).any()
        got_mask = sub.shell_mask.data.cpu().numpy().reshape(rim.shape[::-1]).transpose(2, 1, 0)
        assert np.array_equal(got_mask, rim), r
        assert sub.mesh is None and (sub.shell_mask.datatype, sub.shell_mask.slope, sub.shell_mask.inter) == (2, 1.0, 0.0)
        ref = radiomics.extract(scan, rim, DEV, classes="all", glszm=True, bin_width=25.0)
        a, b = radiomics.unpack_block(sub.block.cpu().numpy()), radiomics.unpack_block(ref.block.cpu().numpy())
        assert a["n"] == b["n"] == int(rim.sum()) and a["n_bins"] == b["n_bins"]
        for key in ("lo", "hi", "moments"):
            assert np.array_equal(a[key], b[key]), key
        assert torch.equal(sub.hist, ref.hist) and torch.equal(sub.glcm, ref.glcm)
        under = radiomics.finish(ref)
        prefix = radiomics.shell_image_type(r)
        cols = [n for n in names if n.startswith(prefix + "_")]
        assert len(cols) == 18 + 23 + 16 + 14 + 5 + 16
        for n in cols:
            v, w = feats[n], under["original_" + n[len(prefix) + 1:]]
            assert (np.isnan(v) and np.isnan(w)) or abs(v - w) <= 64 * 2.0 ** -53 * max(abs(v), abs(w)), (n, v, w)
    # buffers are reused, and only by an extraction of the same widths
    again = radiomics.extract(scan, mask, DEV, shell_mm=[2.5, 5], buffers=res, **kw)
    assert again.shell_workspace.data_ptr() == res.shell_workspace.data_ptr()
    assert again.shell[1][1].shell_mask.data.data_ptr() == res.shell[1][1].shell_mask.data.data_ptr()
    assert again.shell[0][1].block.data_ptr() == res.shell[0][1].block.data_ptr()
    feats2 = radiomics.finish(again)
    assert all(np.array_equal(_bits(feats2[k]), _bits(v)) for k, v in feats.items())
    with pytest.raises(ValueError, match="shell widths"):
        radiomics.extract(scan, mask, DEV, shell_mm=[5], buffers=res, **kw)


def test_the_shell_is_built_on_the_grid_the_extraction_sees():
    scan, mask, _ = _pair(seed=6)
    res = radiomics.extract(scan, mask, DEV, resample=(1.6, 1.8, 3.0), shell_mm=[4.0])
    grid_scan, grid_mask = res.resampled
    assert grid_scan.shape != scan.shape and res.shell[0][1].shape == grid_scan.shape
    spacing = radiomics.spacing_of(grid_scan.affine)
    assert np.allclose(spacing, (1.6, 1.8, 3.0))
    on_grid = grid_mask.data.cpu().numpy().reshape(grid_scan.shape[::-1]).transpose(2, 1, 0)
    rim = M.margin(on_grid, spacing, 4.0, "shell")[0]
    got = res.shell[0][1].shell_mask.data.cpu().numpy().reshape(rim.shape[::-1]).transpose(2, 1, 0)
    assert np.array_equal(got, rim) and rim.sum() > 0
    assert len(radiomics.finish(res)) == 47 + 41


def test_an_empty_shell_raises_as_an_empty_roi_does():
    scan, mask, _ = _pair(seed=7, shape=(12, 10, 6))
    with pytest.raises(ConfigurationError, match=r"shell-5-0-mm: the mask selects no voxel"):
        radiomics.finish(radiomics.extract(scan, np.ones_like(mask), DEV, shell_mm=[5]))
    with pytest.raises(ValueError, match="smaller than every voxel spacing"):
        radiomics.extract(scan, mask, DEV, shell_mm=[0.5])


# ---- the command lines: one fresh process each ---------------------------------------------------------------------------------------------
def _locations(tree, cfg):
    return ["--config", cfg, "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
            "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]


def test_cli_two_epochs_with_a_margin_and_a_cache_then_scan_space_inference(trees, tmp_path):
    """`--mask_margin_mm` with `--cache_volumes` trains the checkpoint that the host-dilated tree trains without the flag, tensor for
    tensor; the inference then writes its maps on the scans' grids, non-zero on the widened box alone."""
    plain, wide = trees
    cfg = tiny_config(tmp_path)
    main = os.path.join(ROOT, "main.py")
    train = ["--images", "--preop", "--survival", "--epochs", "2"]
    (tmp_path / "m").mkdir()
    (tmp_path / "w").mkdir()
    log = process([main, "--output_path", str(tmp_path / "m"), *train, "--mask_margin_mm", str(RADIUS), "--cache_volumes", *_locations(plain, cfg)], tmp_path / "m")
    assert "epoch 2/2" in log and "volume cache: 4 of 4 patients cached" in log
    log = process([main, "--output_path", str(tmp_path / "w"), *train, *_locations(wide, cfg)], tmp_path / "w")
    assert "epoch 2/2" in log
    a, b = (torch.load(tmp_path / d / "best_surv_model.pth", map_location="cpu") for d in ("m", "w"))
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    log = process([main, "--output_path", str(tmp_path / "m"), "--inference", "--images", "--preop", "--survival", "--scan_space", "--mask_margin_mm", str(RADIUS),
                   "--weights", str(tmp_path / "m" / "best_surv_model.pth"), *_locations(plain, cfg)], tmp_path / "m")
    assert "All C-indexes" in log
    from tests import _ingest_ref as R
    uid = int(open(plain["val_uids"]).read().split()[0])
    i = plain["uids"].index(uid)
    d = os.path.join(plain["image_loc"], "t1", f"SYN-{i:04d}-t1-a")
    scan, mask = nifti.read(os.path.join(d, "scan_t1.nii.gz")), nifti.read(os.path.join(d, "mask.nii.gz"))
    h = R.read_nifti_file(tmp_path / "m" / "attention_maps" / f"_patient_{uid}" / "att_map_class0_on_t1.nii.gz")
    assert h["dim"][:4] == (3, *scan.raw.shape)
    kx, ky, kz = S.keep_flags(scan.raw, M.margin(mask.raw, radiomics.spacing_of(scan.affine), RADIUS)[0], (scan.slope, scan.inter))
    box = kx[:, None, None] & ky[None, :, None] & kz[None, None, :]
    assert not np.asarray(h["data"])[~box].any()


def test_cli_radiomics_with_shells_two_epochs_and_the_extraction_tool(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=4, seed=12, val_fraction=0.5)
    cfg = tiny_config(tmp_path, radiomics={"shell_mm": [3]})
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = process([main, "--output_path", str(out), "--radiomics", "--survival", "--epochs", "2", "--shell_mm", "2,4", *_locations(tree, cfg)], out)
    assert "epoch 2/2" in log
    cols, rows = radiomics.read_csv(out / "radiomics_features.csv")
    names = radiomics.feature_names(shell_mm=(2, 4))
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in names] and len(rows) == 4 and cols[-1] == "t2_shell-4-0-mm_glcm_SumSquares"
    tool = tmp_path / "tool.csv"
    log = process(["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--config", cfg, "--out", str(tool)], tmp_path)
    assert f"{2 * (47 + 41)} features" in log                                      # the config's one shell
    tcols, trows = radiomics.read_csv(tool)
    assert tcols[48] == "t1_shell-3-0-mm_firstorder_Energy"
    both = [c for c in tcols if "shell" not in c]
    for r, t in zip(rows, trows):                                                  # the original_* columns do not depend on the shells
        assert [r[cols.index(c)] for c in both] == [t[tcols.index(c)] for c in both]
