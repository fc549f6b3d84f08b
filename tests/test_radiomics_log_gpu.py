"""`mmnn_log_filter` on the device against the numpy restatement (tests/_radiomics_log_ref.py), bit for bit; the `log-sigma-*` columns of
`radiomics.extract` against the existing references fed with the device's own filtered volume; the command lines in fresh processes; and
the MLP at the widths of a table with one scale.

The filter is compared with array equality (NaN equal to NaN): the restatement keeps the kernel's order per output.  The features hold
the tolerances of the files that own them (tests/_radiomics_cases.py, _radiomics_texture_cases.py, _radiomics_zones_cases.py: BOUND), and
their exactness rules, unchanged."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import ingest, synth_nifti
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_log_ref as L
from tests import _radiomics_ref as R
from tests import _radiomics_texture_ref as T
from tests import _radiomics_zones_ref as Z
from tests._radiomics_cases import BOUND, _case
from tests._radiomics_harness import (DEV, GUARD, PATTERN, ROOT, device_bytes, leave_the_dropout_stream_where_it_was, mlp_at_width,  # noqa: F401
                                      process)
from tests._cli import tiny_config
from tests._radiomics_log_cases import FEATURE_CASES, FILTER_CASES, MLP_STREAM, TILE_COLUMNS, TILE_LINE, TILE_ROWS, TILE_X, affine_of
from tests._radiomics_texture_cases import BOUND as TEXTURE_BOUND
from tests._radiomics_zones_cases import BOUND as ZONES_BOUND

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(name):
    """The restatement of a filter case, computed once and shared."""
    if name not in _REF:
        c = FILTER_CASES[name]
        radius, taps, weight = radiomics.log_taps(c["sigma"], c["spacing"])
        assert tuple(radius) == c["radii"]
        _REF[name] = L.restate(c["scan"], radius, taps, weight, c["scale"])
    return _REF[name]


def _call(scan, radius, taps, weight, scale=(1.0, 0.0), lead=0, expect=0, null=None, scan_type=None):
    """One call through the C-ABI itself: `out` sits between guard bytes in a buffer filled with a pattern, the workspace starts from
    0xFF.  Returns (status, out as float32 (x, y, z) or None when nothing may have been written)."""
    x, y, z = scan.shape
    n = x * y * z
    buf = torch.full((GUARD + (n * 4 + 255) // 256 * 256 + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    sbuf, sp = device_bytes(scan, lead)
    nbytes = _lib.lib().mmnn_log_filter_workspace_bytes(x, y, z)
    assert nbytes >= 4 * 8 * n
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    tp = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float64)).to(DEV)
    desc = _lib.LogFilterDesc(x, y, z, ingest.TYPE_CODES[scan.dtype] if scan_type is None else scan_type, float(scale[0]), float(scale[1]),
                              (ctypes.c_int32 * 3)(*[int(r) for r in radius]), (ctypes.c_double * 3)(*[float(w) for w in weight]))
    args = dict(scan=sp, taps=tp.data_ptr(), out=buf.data_ptr() + GUARD, ws=ws.data_ptr())
    if null is not None:
        args[null] = None
    status = _lib.lib().mmnn_log_filter(ctypes.byref(desc), args["scan"], args["taps"], args["out"], args["ws"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status == expect, (status, _lib.last_error())
    b = buf.cpu().numpy()
    if status != 0:
        assert (b == PATTERN).all() and bool((ws == 0xFF).all()), "a refused call wrote something"
        return status, None
    assert (b[:GUARD] == PATTERN).all() and (b[GUARD + n * 4:] == PATTERN).all(), "bytes outside `out` were written"
    return status, b[GUARD:GUARD + n * 4].view(np.float32).reshape((x, y, z), order="F").copy()


def _run(name):
    c = FILTER_CASES[name]
    radius, taps, weight = radiomics.log_taps(c["sigma"], c["spacing"])
    return _call(c["scan"], radius, taps, weight, c["scale"], c["lead"])[1]


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", list(FILTER_CASES))
def test_filter_equals_the_restatement_bit_for_bit(name):
    got, want = _run(name), _ref(name)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 1.0
    bad = int((got != want).sum())
    assert _same(got, want), (name, bad, float(np.abs(got - want).max()))
    c = FILTER_CASES[name]
    if name == "radius_64":
        assert c["radii"][0] == 64 <= _lib.LOG_FILTER_MAX_RADIUS
    if name == "radius_above_extents":
        assert all(r > s for r, s in zip(c["radii"], c["scan"].shape))
    if name == "tiles_xy":                                   # both x tiles, a last column tile of 4, two tiles along y, a last row group of 2
        x, y, z = c["scan"].shape
        assert x > TILE_X and x % TILE_COLUMNS and y > TILE_LINE and (y * z) % TILE_ROWS
    if name == "tiles_z":
        assert c["scan"].shape[2] > TILE_LINE and c["scan"].shape[0] > TILE_COLUMNS


def test_a_nan_poisons_exactly_the_voxels_within_the_radii():
    c = FILTER_CASES["small_radii"]
    radius, taps, weight = radiomics.log_taps(c["sigma"], c["spacing"])
    scan = c["scan"].astype(np.float32)
    at = (6, 5, 4)
    scan[at] = np.nan
    got = _call(scan, radius, taps, weight)[1]
    idx = np.indices(scan.shape)
    box = np.all([np.abs(idx[a] - at[a]) <= int(radius[a]) for a in range(3)], axis=0)
    assert np.array_equal(np.isnan(got), box) and 0 < int(box.sum()) < box.size
    assert _same(got, L.restate(scan, radius, taps, weight))


def test_two_calls_into_different_buffers_agree_bit_for_bit():
    for name in ("larger_radii", "tiles_xy"):
        a, b = _run(name), _run(name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def test_refusals_write_nothing():
    L_ = _lib.lib()
    assert L_.mmnn_log_filter_workspace_bytes(0, 4, 4) == -1 and L_.mmnn_log_filter_workspace_bytes(4, 4, -1) == -1
    assert L_.mmnn_log_filter_workspace_bytes(2048, 1024, 1024) == -1 and L_.mmnn_log_filter_workspace_bytes(13, 10, 9) >= 4 * 8 * 13 * 10 * 9
    c = FILTER_CASES["small_radii"]
    radius, taps, weight = radiomics.log_taps(c["sigma"], c["spacing"])
    big = _lib.LOG_FILTER_MAX_RADIUS + 1
    long_taps = np.zeros(6 * (2 * big + 1))
    for bad in (dict(radius=(0, 4, 1)), dict(radius=(5, big, 1), taps=long_taps), dict(radius=(5, 4, -1)), dict(weight=(1.0, float("nan"), 1.0)),
                dict(weight=(float("inf"), 1.0, 1.0)), dict(null="scan"), dict(null="taps"), dict(null="out"), dict(null="ws"), dict(scan_type=3),
                dict(lead=1)):
        kw = dict(radius=radius, taps=taps, weight=weight)
        kw.update(bad)
        assert _call(c["scan"], kw["radius"], kw["taps"], kw["weight"], expect=1, null=kw.get("null"), scan_type=kw.get("scan_type"),
                     lead=kw.get("lead", 0)) == (1, None), bad
    assert L_.mmnn_log_filter(None, None, None, None, None, None) == 1


# ---- the features of the filtered images ---------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _extract(name, **kw):
    c = FEATURE_CASES[name]
    scan = ingest.upload(c["scan"], torch.device(DEV))
    scan.affine = affine_of(c["spacing"])
    return radiomics.extract(scan, c["mask"], DEV, classes=c["classes"], glszm=c["glszm"], log_sigma=c["sigmas"], log_bin_width=c["bin_width"], **kw)


def _check_first_order_and_glcm(name, im, got, filtered, mask, bin_width, voxel_volume):
    """As tests/test_radiomics_gpu.py: _compare holds the device's block to the restatement of the same (scan, mask)."""
    with np.errstate(all="ignore"):
        ref = R.restate(filtered, mask, bin_width, 256, (1.0, 0.0), (1.0, 0.0))
    assert not (ref["empty"] or ref["nonfinite"] or ref["overflow"]) and 8 <= ref["n_bins"] <= 256
    exact = R.exact(ref)
    for k in R.BITWISE:
        cls = "firstorder" if k in R.FIRSTORDER else "glcm"
        assert _same_bits(got[f"{im}_{cls}_{k}"], ref["firstorder"][k][0]), (name, im, k)
    values = {k: R.value_and_scale(ref, k)[0] for names in R.CLASSES.values() for k in names}
    mine = {k: float(got[f"{im}_{'firstorder' if k in R.FIRSTORDER else 'glcm'}_{k}"]) for k in values}
    dev = R.deviations(ref, mine, exact)
    print(name, im, "Ng", ref["n_bins"], "device", {k: f"{v / 2 ** -53:.2f}" for k, v in dev.items()})
    for cls in R.CLASSES:
        assert dev[cls] <= BOUND[cls], (name, im, cls, dev[cls] / 2 ** -53)
    assert got[f"{im}_firstorder_TotalEnergy"] == got[f"{im}_firstorder_Energy"] * voxel_volume
    return ref


@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_log_columns_equal_the_references_on_the_devices_filtered_volume(name):
    c = FEATURE_CASES[name]
    res = _extract(name)
    feats = radiomics.finish(res)
    names = radiomics.feature_names(c["classes"], c["glszm"], False, c["sigmas"])
    assert list(feats) == list(names) and [s for s, _ in res.log] == sorted(c["sigmas"])
    n_orig = len(radiomics.feature_names(c["classes"], c["glszm"]))
    assert not any("shape" in k for k in names[n_orig:]) and len(names) == n_orig + len(c["sigmas"]) * (n_orig - 6)
    volume = float(np.prod(c["spacing"]))
    x, y, z = c["scan"].shape
    for sigma, sub in res.log:
        im = radiomics.log_image_type(sigma)
        assert sub.image == im and sub.filtered.datatype == 16 and sub.filtered.slope == 0.0 and sub.bin_width == c["bin_width"]
        filtered = sub.filtered.data.view(torch.float32).cpu().numpy().reshape((x, y, z), order="F")
        radius, taps, weight = radiomics.log_taps(sigma, c["spacing"])
        assert _same(filtered, L.restate(c["scan"], radius, taps, weight))                      # the spacing came from the affine
        _check_first_order_and_glcm(name, im, feats, filtered, c["mask"], c["bin_width"], volume)
        case = _case(filtered, c["mask"], bin_width=c["bin_width"])
        if c["classes"]:
            assert c["classes"] == radiomics.TEXTURE_CLASSES                                     # T.deviations runs over all three
            tex = T.restate(case)
            assert not tex["flagged"]
            values = {cls: {k: feats[f"{im}_{cls}_{k}"] for k in tex["features"][cls]} for cls in c["classes"]}
            for cls in c["classes"]:
                for k, (want, _) in tex["features"][cls].items():
                    assert math.isnan(want) == math.isnan(values[cls][k]), (name, im, cls, k)
                    if cls == "ngtdm" and want in (0.0, 1.0e6):
                        assert values[cls][k] == want                                            # the special values are exact
            dev = T.deviations(tex, values, T.exact(tex))
            print(name, im, "texture", {k: f"{v / 2 ** -53:.2f}" for k, v in dev.items()})
            for cls in T.CLASSES:
                assert dev[cls] <= TEXTURE_BOUND[cls], (name, im, cls, dev[cls] / 2 ** -53)
        if c["glszm"]:
            zn = Z.restate(case)
            assert not zn["flagged"]
            values = {k: feats[f"{im}_glszm_{k}"] for k in Z.GLSZM}
            dev = Z.deviations(zn, values, Z.exact(zn))
            for cls in Z.CLASSES:
                assert dev[cls] <= ZONES_BOUND[cls], (name, im, cls, dev[cls] / 2 ** -53)


def test_original_columns_are_those_of_a_run_without_log_sigma_and_buffers_are_reused():
    c = FEATURE_CASES["every_class"]
    scan = ingest.upload(c["scan"], torch.device(DEV))
    scan.affine = affine_of(c["spacing"])
    plain = radiomics.extract(scan, c["mask"], DEV, classes=c["classes"], glszm=True, mesh=True)
    res = _extract("every_class", mesh=True)
    assert plain.log == () and plain.filter_workspace is None and len(res.log) == 1 and res.log[0][1].mesh is None
    for k in ("block", "hist", "glcm", "texture", "glrlm", "gldm", "ngtdm_n", "ngtdm_s", "zones", "labels", "sizes", "levels", "mesh", "mesh_cfg"):
        assert torch.equal(getattr(plain, k), getattr(res, k)), k
    want, feats = radiomics.finish(plain), radiomics.finish(res)
    assert list(feats)[:len(want)] == list(want) == list(radiomics.feature_names("all", True, True)) and len(feats) == 106 + 92
    assert all(_same_bits(feats[k], v) for k, v in want.items())
    again = _extract("every_class", mesh=True, buffers=res)
    sub, sub2 = res.log[0][1], again.log[0][1]
    assert again.block.data_ptr() == res.block.data_ptr() and again.filter_workspace.data_ptr() == res.filter_workspace.data_ptr()
    assert sub2.block.data_ptr() == sub.block.data_ptr() and sub2.filtered.data.data_ptr() == sub.filtered.data.data_ptr()
    assert sub2.filter_taps.data_ptr() == sub.filter_taps.data_ptr() and sub2.zones.data_ptr() == sub.zones.data_ptr()
    feats2 = radiomics.finish(again)
    assert list(feats2) == list(feats) and all(_same_bits(feats2[k], v) for k, v in feats.items())
    with pytest.raises(ValueError, match="scales"):
        radiomics.extract(scan, c["mask"], DEV, classes=c["classes"], glszm=True, mesh=True, log_sigma=(2.0,), buffers=res)
    vol = radiomics.log_filter(scan, 5.0, DEV)
    assert torch.equal(vol.data, sub.filtered.data) and vol.affine is scan.affine and (vol.datatype, vol.slope) == (16, 0.0)


def test_a_flag_on_a_filtered_image_names_the_image_type():
    c = FEATURE_CASES["default_two_scales"]
    with pytest.raises(ConfigurationError, match=r"log-sigma-1-0-mm-3D.*log\.bin_width"):
        radiomics.finish(radiomics.extract(c["scan"], c["mask"], DEV, log_sigma=(1.0,), log_bin_width=0.01))
    with pytest.raises(ConfigurationError, match="x axis"):
        radiomics.extract(c["scan"], c["mask"], DEV, log_sigma=(0.1,))


# ---- the MLP at the widths of a table with one scale ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [88, 176])
def test_mlp_at_log_width_vs_fp64(width):
    """MLP(width) forward and backward at N = 4, training mode, against the fp64 torch restatement, at the bar tests/test_tail_ops_gpu.py
    holds width 32 to: 47 + 41 columns of one modality with one scale, 176 of two."""
    mlp_at_width(width, MLP_STREAM[width])


# ---- the command lines: one fresh process each -----------------------------------------------------------------------------------------------
def test_cli_extraction_tool_with_log_sigma_writes_the_rows_of_finish(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=11)
    names = radiomics.feature_names(log_sigma=(1, 3))
    out = tmp_path / "radiomics.csv"
    log = process(["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--log_sigma", "1,3", "--out", str(out)],
                   tmp_path)
    assert "258 features" in log
    cols, rows = radiomics.read_csv(out)
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in names] and len(cols) == 1 + 2 * (47 + 2 * 41) and len(rows) == 3
    assert cols[48] == "t1_log-sigma-1-0-mm-3D_firstorder_Energy" and cols[-1] == "t2_log-sigma-3-0-mm-3D_glcm_SumSquares"
    ds = ImageDataset(os.path.join(tree["image_loc"], "t1"), tree["key_loc"])
    part = radiomics.extract_tree(ds, DEV, log_sigma=(3, 1))                                     # one stacked read-back per batch
    assert list(part[0]) == ["MRN"] + list(names)
    for k, p in enumerate(ds.patients):
        want = radiomics.finish(radiomics.extract(*ds._load(p), DEV, log_sigma=(1, 3)))
        row = next(r for r in rows if int(r[0]) == ds._uid_of(p))
        for n, v in want.items():
            assert float(row[cols.index(f"t1_{n}")]) == v == part[k][n] or math.isnan(v), (p, n)


def test_cli_trains_on_the_log_table_then_infers_with_the_saved_scaler(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=12, val_fraction=0.34)
    loc = ["--config", tiny_config(tmp_path), "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = process([main, "--output_path", str(out), "--radiomics", "--survival", "--image_loc", tree["image_loc"], "--log_sigma", "1,3",
                    "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    for name in ("radiomics_features.csv", "radiomics_scaler.csv", "best_surv_model.pth"):
        assert (out / name).exists(), name
    cols, rows = radiomics.read_csv(out / "radiomics_features.csv")
    assert len(cols) == 1 + 2 * (47 + 2 * 41) and cols[-1] == "t2_log-sigma-3-0-mm-3D_glcm_SumSquares" and len(rows) == 6
    log = process([main, "--output_path", str(out), "--inference", "--radiomics", "--survival", "--weights", str(out / "best_surv_model.pth"),
                    "--rad_loc", str(out / "radiomics_features.csv"), *loc], out)
    assert "All C-indexes" in log
