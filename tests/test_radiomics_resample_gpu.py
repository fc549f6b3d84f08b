"""`mmnn_normalize_scan` and `mmnn_resample_pair` on the device against the numpy restatement (tests/_radiomics_resample_ref.py), bit for
bit; `radiomics.extract(..., normalize=..., resample=...)` against the existing references fed with the device's own resampled pair;
the switches off; the buffers; and the command lines in fresh processes.

The volumes are compared with array equality (NaN equal to NaN): the restatement keeps the kernels' order per output.  The device's mean
and sd are held to BOUND["firstorder_moment"] of tests/_radiomics_cases.py, the bar and the scales first-order Mean and Variance hold
(the mean relative to the mean |v|, the variance sd^2 relative to itself), and `out` to the
restatement fed those.  The features hold the tolerances of the files that own them and their exactness rules, unchanged."""
import ctypes
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import ingest, synth_nifti
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_log_ref as LG
from tests import _radiomics_mesh_ref as M
from tests import _radiomics_ref as R
from tests import _radiomics_resample_ref as P
from tests import _radiomics_texture_ref as T
from tests import _radiomics_zones_ref as Z
from tests._radiomics_cases import BOUND, _case
from tests._radiomics_harness import (DEV, GUARD, PATTERN, ROOT, device_bytes, guarded, cut, leave_the_dropout_stream_where_it_was,  # noqa: F401
                                      process)
from tests._cli import tiny_config
from tests._radiomics_mesh_cases import BOUND as MESH_BOUND
from tests._radiomics_resample_cases import (BIN_WIDTH, FEATURE_CASES, LINE_BATCH, LINE_TPB, NORM_BATCH, NORM_MAX_PARTS, NORM_TPB, NORM_WRITE_GROUPS,
                                             NORMALIZE_CASES, RESAMPLE_CASES, SCALE, X_CHUNK, X_LINES, Z_RUN, affine_of)
from tests._radiomics_texture_cases import BOUND as TEXTURE_BOUND
from tests._radiomics_zones_cases import BOUND as ZONES_BOUND

pytestmark = pytest.mark.gpu
K = radiomics.resample_constants()
_REF = {}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---- normalisation ----------------------------------------------------------------------------------------------------------------------------
def _normalize(scan, scale=(1.0, 0.0), lead=0, factor=SCALE, outliers=0.0, expect=0, null=None, scan_type=None, shift=None):
    """One call through the C-ABI itself: `out` and the result block sit between guard bytes in a buffer filled with a pattern, the
    workspace starts from 0xFF.  Returns (out as float32 (x, y, z), the unpacked block), or None once a refusal has written nothing."""
    x, y, z = scan.shape
    n = x * y * z
    sizes = [n * 4, _lib.NORMALIZE_RESULT_BYTES]
    buf, offs = guarded(sizes)
    sbuf, sp = device_bytes(scan, lead)
    nbytes = _lib.lib().mmnn_normalize_scan_workspace_bytes(x, y, z)
    assert nbytes > 0
    ws = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    desc = _lib.NormalizeDesc(x, y, z, ingest.TYPE_CODES[scan.dtype] if scan_type is None else scan_type, float(scale[0]), float(scale[1]),
                              float(factor), float(outliers))
    args = dict(scan=sp, out=buf.data_ptr() + offs[0], result=buf.data_ptr() + offs[1], ws=ws.data_ptr())
    if null is not None:
        args[null] = None
    if shift is not None:
        args[shift[0]] += shift[1]
    status = _lib.lib().mmnn_normalize_scan(ctypes.byref(desc), args["scan"], args["out"], args["result"], args["ws"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status == expect, (status, _lib.last_error())
    if status != 0:
        assert bool((buf == PATTERN).all()) and bool((ws == 0xFF).all()), "a refused call wrote something"
        return None
    out, block = cut(buf, offs, sizes, "bytes outside `out` and the result block were written")
    assert bool((ws[nbytes:] == 0xFF).all()), "bytes behind the workspace were written"
    return out.view(np.float32).reshape((x, y, z), order="F").copy(), radiomics.unpack_normalize(block)


@pytest.mark.parametrize("outliers", [0.0, 3.0, 1.0])                   # (a uniform scan never leaves 3 sd: 1 is where the clamp acts on every case)
@pytest.mark.parametrize("name", list(NORMALIZE_CASES))
def test_normalisation_equals_the_restatement_fed_the_devices_statistics(name, outliers):
    c = NORMALIZE_CASES[name]
    got, st = _normalize(c["scan"], c["scale"], c["lead"], outliers=outliers)
    n, mean, sd = P.normalize_stats(c["scan"], c["scale"])
    v = P.scaled(c["scan"], c["scale"])
    rel = {"mean": abs(st["mean"] - mean) / float(np.abs(v).sum() / n), "variance": abs(st["sd"] ** 2 - sd ** 2) / sd ** 2}
    print(name, "n", n, "deviation / 2^-53", {k: f"{e / 2 ** -53:.2f}" for k, e in rel.items()})
    assert st["n"] == n and not st["nonfinite"] and max(rel.values()) <= BOUND["firstorder_moment"], (name, rel)
    want = P.normalize(c["scan"], c["scale"], SCALE, outliers, st["mean"], st["sd"])
    assert np.isfinite(want).all() and _same(got, want), (name, int((got != want).sum()))
    if outliers:
        assert float(np.abs(got).max()) <= outliers * SCALE
    if outliers == 1.0:
        assert int((got == SCALE).sum()) > 1 and int((got == -SCALE).sum()) > 1
    if name == "two_trips":
        assert n > NORM_TPB * NORM_MAX_PARTS
    if name == "batched_strides":                            # the batched loops of all three passes, each with a tail behind it
        assert n > NORM_BATCH * NORM_WRITE_GROUPS * NORM_TPB > (NORM_BATCH - 1) * NORM_MAX_PARTS * NORM_TPB
        assert n % (NORM_BATCH * NORM_WRITE_GROUPS * NORM_TPB) and n % (NORM_BATCH * NORM_MAX_PARTS * NORM_TPB)


def test_normalisation_twice_agrees_bit_for_bit():
    for name in ("int16", "two_trips"):
        c = NORMALIZE_CASES[name]
        (a, sa), (b, sb) = _normalize(c["scan"]), _normalize(c["scan"])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and sa == sb, name


def test_a_nan_voxel_and_a_constant_scan_give_nan_everywhere():
    scan = NORMALIZE_CASES["float32"]["scan"].copy()
    scan[3, 4, 5] = np.nan
    got, st = _normalize(scan, outliers=3.0)
    assert np.isnan(got).all() and st["nonfinite"] and math.isnan(st["mean"]) and _same(got, P.normalize(scan, mean=st["mean"], sd=st["sd"], outliers=3.0))
    scan[3, 4, 5] = np.inf
    got, st = _normalize(scan)
    assert np.isnan(got).all() and st["nonfinite"]
    got, st = _normalize(np.full((13, 10, 9), 7, np.int16))
    assert np.isnan(got).all() and not st["nonfinite"] and st["mean"] == 7.0 and st["sd"] == 0.0
    with pytest.raises(ConfigurationError, match="normalize"):
        radiomics.finish(radiomics.extract(np.full((13, 10, 9), 7, np.int16), FEATURE_CASES["anisotropic_to_1mm"]["mask"], DEV, normalize=True))


def test_normalisation_refusals_write_nothing():
    scan = NORMALIZE_CASES["int16"]["scan"]
    for bad in (dict(factor=0.0), dict(factor=-1.0), dict(factor=float("nan")), dict(factor=float("inf")), dict(outliers=-1.0), dict(outliers=float("nan")),
                dict(outliers=float("inf")), dict(null="scan"), dict(null="out"), dict(null="result"), dict(null="ws"), dict(scan_type=3), dict(lead=1),
                dict(shift=("out", 2)), dict(shift=("result", 4)), dict(shift=("ws", 64))):
        assert _normalize(scan, expect=1, **bad) is None, bad
    assert _lib.lib().mmnn_normalize_scan(None, None, None, None, None, None) == 1 and "null" in _lib.last_error()
    with pytest.raises(ValueError, match="extent"):
        _lib.check(_lib.lib().mmnn_normalize_scan(ctypes.byref(_lib.NormalizeDesc(0, 4, 4, 4, 1.0, 0.0, 100.0, 0.0)), 1, 1, 1, 1, None), "normalize")


# ---- resampling -------------------------------------------------------------------------------------------------------------------------------
def _grid(c):
    g = radiomics.resample_grid(c["scan"].shape, affine_of(c["spacing"]), c["to"])
    assert g.shape == c["out"]
    return g, radiomics.resample_tables(c["scan"].shape, g)


def _resample(scan, mask, grid, tables, scale=(1.0, 0.0), lead=0, expect=0, null=None, types=None, shift=None, device_tables=None, constants=None,
              extents=None):
    """One call through the C-ABI itself: `out` and `out_mask` between guard bytes in a buffer filled with a pattern, the workspace
    started at 0xFF with guard bytes behind it.  Returns (scan float32, mask uint8), or None once a refusal has written nothing."""
    (x, y, z), (mx, my, mz) = scan.shape, grid.shape
    m = mx * my * mz
    sizes = [m * 4, m]
    buf, offs = guarded(sizes)
    sbuf, sp = device_bytes(scan, lead)
    mbuf, mp = device_bytes(mask, 0)
    nbytes = _lib.lib().mmnn_resample_pair_workspace_bytes(x, y, z, mx, my, mz)
    assert nbytes >= 8 * (x * y * z + mx * y * z + mx * my * z)
    ws = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    host = np.ascontiguousarray(tables)
    tp = torch.from_numpy((host if device_tables is None else device_tables).view(np.uint8).copy()).to(DEV)
    k = dict(K, **(constants or {}))
    stype, mtype = types or (ingest.TYPE_CODES[scan.dtype], ingest.TYPE_CODES[mask.dtype])
    desc = _lib.ResampleDesc(*(extents or (x, y, z, mx, my, mz)), stype, mtype, float(scale[0]), float(scale[1]), 1.0, 0.0, k["pole"], k["pole_gain"], k["gain"],
                             (ctypes.c_double * _lib.RESAMPLE_HORIZON)(*np.asarray(k["pole_power"]).tolist()))
    args = dict(scan=sp, mask=mp, tables_host=host.ctypes.data, tables=tp.data_ptr(), out=buf.data_ptr() + offs[0], out_mask=buf.data_ptr() + offs[1], ws=ws.data_ptr())
    if null is not None:
        args[null] = None
    if shift is not None:
        args[shift[0]] += shift[1]
    status = _lib.lib().mmnn_resample_pair(ctypes.byref(desc), *(args[a] for a in ("scan", "mask", "tables_host", "tables", "out", "out_mask", "ws")),
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status == expect, (status, _lib.last_error())
    if status != 0:
        assert bool((buf == PATTERN).all()) and bool((ws == 0xFF).all()), "a refused call wrote something"
        return None
    out, om = cut(buf, offs, sizes, "bytes outside `out` and `out_mask` were written")
    assert bool((ws[nbytes:] == 0xFF).all()), "bytes behind the workspace were written"
    return out.view(np.float32).reshape(grid.shape, order="F").copy(), om.reshape(grid.shape, order="F").copy()


def _run(name):
    c = RESAMPLE_CASES[name]
    g, t = _grid(c)
    return _resample(c["scan"], c["mask"], g, t, c["scale"], c["lead"])


def _ref(name):
    """The restatement of a resample case, computed once and shared."""
    if name not in _REF:
        c = RESAMPLE_CASES[name]
        g, t = _grid(c)
        _REF[name] = P.restate(c["scan"], c["mask"], g, t, K, c["scale"]) + (P.inside_of(g.shape, t),)
    return _REF[name]


@pytest.mark.parametrize("name", list(RESAMPLE_CASES))
def test_resampling_equals_the_restatement_bit_for_bit(name):
    (got, gm), (want, wm, inside) = _run(name), _ref(name)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 1.0 and 0 < int(wm.sum()) < wm.size
    assert _same(got, want), (name, int((got != want).sum()), float(np.abs(got - want).max()))
    assert _same(gm, wm), (name, int((gm != wm).sum()))
    assert not got[~inside].any() and not gm[~inside].any() and set(np.unique(gm)) <= {0, 1}
    x, y, z = RESAMPLE_CASES[name]["scan"].shape
    if name == "longer_than_horizon":
        assert x > _lib.RESAMPLE_HORIZON and X_CHUNK < x < 2 * X_CHUNK
    if name == "axis_kept":
        assert got.shape[2] == z and int((~inside).sum()) == 99
    if name == "anisotropic_to_1mm":                         # 45 output planes: two whole runs of the z gather and one of 13; y = 10 and
        assert int((~inside).sum()) == 495                   # z = 9 samples per line: a whole batch of the y / z prefilter's loads and a tail
        assert got.shape[2] > 2 * Z_RUN and got.shape[2] % Z_RUN and LINE_BATCH < y - 1 < 2 * LINE_BATCH and z - 1 == LINE_BATCH
    if name == "chunk_65":
        assert x == X_CHUNK + 1
    if name == "chunk_128":
        assert x == 2 * X_CHUNK
    if name == "tiles":
        assert x > X_CHUNK and y * z > X_LINES and (y * z) % X_LINES and x * z > LINE_TPB and x * y > LINE_TPB
        assert all(n % LINE_TPB for n in (got.shape[0] * y * z, got.shape[0] * got.shape[1] * z, got.size))
    if name == "extent_1":
        assert z == 1 and got.shape[2] == 2


def test_resampling_twice_agrees_bit_for_bit():
    for name in ("anisotropic_to_1mm", "tiles"):
        (a, am), (b, bm) = _run(name), _run(name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(am, bm), name


def test_restatement_and_device_agree_on_a_scan_with_one_nan():
    c = RESAMPLE_CASES["to_2mm"]
    g, t = _grid(c)
    scan = c["scan"].astype(np.float32)
    scan[6, 5, 4] = np.nan
    mask = c["mask"].astype(np.float32)
    mask[0, 0, 0] = np.nan                                   # a NaN in the mask counts as not 0
    got, gm = _resample(scan, mask, g, t)
    want, wm = P.restate(scan, mask, g, t, K)
    inside = P.inside_of(g.shape, t)
    assert _same(got, want) and _same(gm, wm) and np.isnan(got[inside]).any() and not got[~inside].any() and gm[0, 0, 0] == 1


def test_resampling_refusals_write_nothing():
    c = RESAMPLE_CASES["to_2mm"]
    g, t = _grid(c)
    x, y, z = c["scan"].shape
    far, neg, nan_w, near = t.copy(), t.copy(), t.copy(), t.copy()
    far["i"][g.shape[0] + 1, 3] = y                          # an index one past the y axis
    neg["i"][0, 0] = -1
    nan_w["w"][-1, 2] = np.nan
    near["nearest"][2] = x
    power = np.array(K["pole_power"])
    power[7] = np.inf
    for bad in (dict(tables=far), dict(tables=neg), dict(tables=nan_w), dict(tables=near), dict(null="scan"), dict(null="mask"), dict(null="tables_host"),
                dict(null="tables"), dict(null="out"), dict(null="out_mask"), dict(null="ws"), dict(types=(3, 2)), dict(types=(4, 5)), dict(lead=1),
                dict(shift=("out", 2)), dict(shift=("tables", 4)), dict(shift=("ws", 64)), dict(constants={"pole": float("nan")}),
                dict(constants={"pole_power": power}), dict(extents=(0, y, z) + g.shape), dict(extents=(x, y, z, g.shape[0], -1, g.shape[2])),
                dict(extents=(2048, 1024, 1024) + g.shape), dict(extents=(x, y, z, 2048, 1024, 1024))):
        kw = dict(bad)
        tables = kw.pop("tables", t)
        assert _resample(c["scan"], c["mask"], g, tables, expect=1, device_tables=t, **kw) is None, bad
    assert _lib.lib().mmnn_resample_pair(None, None, None, None, None, None, None, None, None) == 1 and "null" in _lib.last_error()


# ---- the features behind the pre-steps --------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _on_grid(c):
    return dataclasses.replace(ingest.upload(c["scan"], torch.device(DEV)), affine=affine_of(c["spacing"], (-12.0, 7.0, 3.0)))


def _extract(name, **kw):
    c = FEATURE_CASES[name]
    args = dict(classes=c["classes"], glszm=c["glszm"], mesh=c["mesh"], log_sigma=c["sigmas"], log_bin_width=c["log_bin_width"],
                normalize={"scale": SCALE}, resample={"spacing": list(c["to"])})
    args.update(kw)
    return radiomics.extract(_on_grid(c), c["mask"], DEV, **args)


def _host(vol, dtype):
    return vol.data.view(dtype).cpu().numpy().reshape(vol.shape, order="F")


def _check_first_order_and_glcm(name, im, got, scan, mask, bin_width, voxel_volume):
    """As tests/test_radiomics_log_gpu.py: the device's columns against the restatement of the same (scan, mask) at its own bounds."""
    with np.errstate(all="ignore"):
        ref = R.restate(scan, mask, bin_width, 256, (1.0, 0.0), (1.0, 0.0))
    assert not (ref["empty"] or ref["nonfinite"] or ref["overflow"]) and 8 <= ref["n_bins"] <= 256 and ref["n"] >= 16
    exact = R.exact(ref)
    for k in R.BITWISE:
        cls = "firstorder" if k in R.FIRSTORDER else "glcm"
        assert _same_bits(got[f"{im}_{cls}_{k}"], ref["firstorder"][k][0]), (name, im, k)
    values = {k: R.value_and_scale(ref, k)[0] for names in R.CLASSES.values() for k in names}
    mine = {k: float(got[f"{im}_{'firstorder' if k in R.FIRSTORDER else 'glcm'}_{k}"]) for k in values}
    dev = R.deviations(ref, mine, exact)
    print(name, im, "Ng", ref["n_bins"], "ROI", ref["n"], "device", {k: f"{v / 2 ** -53:.2f}" for k, v in dev.items()})
    for cls in R.CLASSES:
        assert dev[cls] <= BOUND[cls], (name, im, cls, dev[cls] / 2 ** -53)
    assert got[f"{im}_firstorder_TotalEnergy"] == got[f"{im}_firstorder_Energy"] * voxel_volume
    return ref


def _check_classes(name, im, feats, c, case):
    if c["classes"]:
        assert c["classes"] == radiomics.TEXTURE_CLASSES                                         # T.deviations runs over all three
        tex = T.restate(case)
        assert not tex["flagged"]
        values = {cls: {k: feats[f"{im}_{cls}_{k}"] for k in tex["features"][cls]} for cls in c["classes"]}
        for cls in c["classes"]:
            for k, (want, _) in tex["features"][cls].items():
                assert math.isnan(want) == math.isnan(values[cls][k]), (name, im, cls, k)
                if cls == "ngtdm" and want in (0.0, 1.0e6):
                    assert values[cls][k] == want                                                # the special values are exact
        dev = T.deviations(tex, values, T.exact(tex))
        for cls in T.CLASSES:
            assert dev[cls] <= TEXTURE_BOUND[cls], (name, im, cls, dev[cls] / 2 ** -53)
    if c["glszm"]:
        zn = Z.restate(case)
        assert not zn["flagged"]
        dev = Z.deviations(zn, {k: feats[f"{im}_glszm_{k}"] for k in Z.GLSZM}, Z.exact(zn))
        for cls in Z.CLASSES:
            assert dev[cls] <= ZONES_BOUND[cls], (name, im, cls, dev[cls] / 2 ** -53)


@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_columns_equal_the_references_on_the_devices_resampled_pair(name):
    c = FEATURE_CASES[name]
    res = _extract(name)
    feats = radiomics.finish(res)
    assert list(feats) == list(radiomics.feature_names(c["classes"], c["glszm"], c["mesh"], c["sigmas"]))
    src = affine_of(c["spacing"], (-12.0, 7.0, 3.0))
    g = radiomics.resample_grid(c["scan"].shape, src, c["to"])
    assert res.shape == g.shape and np.array_equal(res.affine, g.affine) and res.source_shape == c["scan"].shape
    assert res.normalize == (SCALE, 0.0) and res.resample == c["to"] and res.resampled[0].datatype == 16 and res.resampled[1].datatype == 2
    st = radiomics.unpack_normalize(res.normalize_block.cpu().numpy())
    normalized = _host(res.normalized, torch.float32)
    assert _same(normalized, P.normalize(c["scan"], scale=SCALE, mean=st["mean"], sd=st["sd"]))
    scan, mask = _host(res.resampled[0], torch.float32), _host(res.resampled[1], torch.uint8)
    want, wm = P.restate(normalized, c["mask"], g, radiomics.resample_tables(c["scan"].shape, g), K)
    assert _same(scan, want) and _same(mask, wm)                                                 # normalise first, then resample
    volume = abs(float(np.linalg.det(g.affine[:3, :3])))
    assert volume == pytest.approx(float(np.prod([t or s for t, s in zip(c["to"], c["spacing"])])), rel=1e-14)
    _check_first_order_and_glcm(name, "original", feats, scan, mask, BIN_WIDTH, volume)
    for k, v in R.shape_reference(mask != 0, g.affine[:3, :3]).items():                          # the shape columns come from the new affine
        assert feats[f"original_shape_{k}"] == pytest.approx(v, rel=1e-12), k
    _check_classes(name, "original", feats, c, _case(scan, mask, bin_width=BIN_WIDTH))
    if c["mesh"]:
        assert np.array_equal(res.linear, g.affine[:3, :3])
        ms, dev = M.restate(mask != 0, g.affine[:3, :3]), radiomics.unpack_mesh(res.mesh.cpu().numpy())
        assert np.array_equal(res.mesh_cfg.cpu().numpy(), ms["cfg"]) and {k: dev[k] for k in M.INTEGERS} == {k: ms[k] for k in M.INTEGERS}
        assert dev["q"].view(np.uint64).tolist() == ms["q"].view(np.uint64).tolist()
        assert M.area_deviation(dev["area"], ms["cfg"], ms["L"]) <= MESH_BOUND
        derived = M.derived(ms["volume48"], dev["area"], ms["q"], g.affine[:3, :3])
        assert [feats[f"original_shape_{n}"] for n in M.MESH_SHAPE] == pytest.approx([derived[n] for n in M.MESH_SHAPE], rel=8 * 2.0 ** -53)
    assert [s for s, _ in res.log] == sorted(c["sigmas"])
    for sigma, sub in res.log:
        im = radiomics.log_image_type(sigma)
        filtered = _host(sub.filtered, torch.float32)
        radius, taps, weight = radiomics.log_taps(sigma, radiomics.spacing_of(g.affine))         # the taps follow the NEW spacing
        assert tuple(radius) == (8, 8, 8) and _same(filtered, LG.restate(scan, radius, taps, weight))
        _check_first_order_and_glcm(name, im, feats, filtered, mask, c["log_bin_width"], volume)
        _check_classes(name, im, feats, c, _case(filtered, mask, bin_width=c["log_bin_width"]))


def test_each_pre_step_alone_and_a_skipped_resampling():
    c = FEATURE_CASES["anisotropic_to_1mm"]
    scan = _on_grid(c)
    plain = radiomics.extract(scan, c["mask"], DEV)
    alone = radiomics.extract(scan, c["mask"], DEV, normalize={"scale": SCALE, "outliers": 1.0})
    assert alone.resampled is None and alone.shape == c["scan"].shape and alone.affine is scan.affine and alone.normalize == (SCALE, 1.0)
    st = radiomics.unpack_normalize(alone.normalize_block.cpu().numpy())
    assert _same(_host(alone.normalized, torch.float32), P.normalize(c["scan"], scale=SCALE, outliers=1.0, mean=st["mean"], sd=st["sd"]))
    vol, stats = radiomics.normalize_scan(scan, DEV, SCALE, 1.0)
    assert torch.equal(vol.data, alone.normalized.data) and torch.equal(stats, alone.normalize_block) and vol.affine is scan.affine
    only = radiomics.extract(scan, c["mask"], DEV, resample=1.0)
    g = radiomics.resample_grid(c["scan"].shape, scan.affine, 1.0)
    want, wm = P.restate(c["scan"], c["mask"], g, radiomics.resample_tables(c["scan"].shape, g), K)
    assert only.normalized is None and _same(_host(only.resampled[0], torch.float32), want) and _same(_host(only.resampled[1], torch.uint8), wm)
    pair = radiomics.resample_pair(scan, c["mask"], DEV, 1.0)
    assert torch.equal(pair[0].data, only.resampled[0].data) and torch.equal(pair[1].data, only.resampled[1].data) and np.array_equal(pair[0].affine, g.affine)
    skipped = radiomics.extract(scan, c["mask"], DEV, resample=c["spacing"])                     # every ratio 1: the step is skipped
    assert skipped.resampled is None and skipped.resample == c["spacing"] and skipped.pre_workspace is None
    for k in ("block", "hist", "glcm"):
        assert torch.equal(getattr(skipped, k), getattr(plain, k)), k
    assert radiomics.resample_pair(scan, c["mask"], DEV, 0)[0] is scan


def test_switches_off_change_nothing():
    c = FEATURE_CASES["every_class_to_half_mm"]
    scan = _on_grid(c)
    kw = dict(classes=c["classes"], glszm=True, mesh=True, log_sigma=(2.0,))
    plain = radiomics.extract(scan, c["mask"], DEV, **kw)
    off = radiomics.extract(scan, c["mask"], DEV, normalize=None, resample=None, **kw)
    off2 = radiomics.extract(scan, c["mask"], DEV, normalize=False, **kw)
    for r in (plain, off, off2):
        for k in ("normalize", "normalized", "normalize_block", "resample", "resampled", "resample_tables", "pre_workspace", "source_shape"):
            assert getattr(r, k) is None, k
        assert r.shape == c["scan"].shape and r.affine is scan.affine
    for r in (off, off2):
        for a, b in ((plain, r), (plain.log[0][1], r.log[0][1])):
            for k in ("block", "hist", "glcm", "texture", "glrlm", "gldm", "ngtdm_n", "ngtdm_s", "zones", "labels", "sizes", "levels"):
                assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert torch.equal(plain.mesh, r.mesh) and torch.equal(plain.mesh_cfg, r.mesh_cfg)
        assert torch.equal(plain.log[0][1].filtered.data, r.log[0][1].filtered.data)
    want, got = radiomics.finish(plain), radiomics.finish(off)
    assert list(want) == list(got) and all(_same_bits(got[k], v) for k, v in want.items())


def test_buffers_are_reused_and_other_settings_or_extents_are_refused():
    c = FEATURE_CASES["every_class_to_half_mm"]
    res = _extract("every_class_to_half_mm")
    feats = radiomics.finish(res)
    again = _extract("every_class_to_half_mm", buffers=res)
    for k in ("block", "hist", "glcm", "workspace", "texture", "zones", "labels", "mesh", "mesh_cfg", "normalize_block", "resample_tables", "pre_workspace",
              "filter_workspace"):
        assert getattr(again, k).data_ptr() == getattr(res, k).data_ptr(), k
    assert again.normalized.data.data_ptr() == res.normalized.data.data_ptr()
    assert again.resampled[0].data.data_ptr() == res.resampled[0].data.data_ptr() and again.resampled[1].data.data_ptr() == res.resampled[1].data.data_ptr()
    assert again.log[0][1].filtered.data.data_ptr() == res.log[0][1].filtered.data.data_ptr()
    feats2 = radiomics.finish(again)
    assert list(feats2) == list(feats) and all(_same_bits(feats2[k], v) for k, v in feats.items())
    for other in (dict(normalize={"scale": 50.0}), dict(normalize=None), dict(resample=0.75), dict(resample=None), dict(normalize={"scale": SCALE, "outliers": 3})):
        with pytest.raises(ValueError, match="pre-steps"):
            _extract("every_class_to_half_mm", buffers=res, **other)
    small = FEATURE_CASES["to_2mm"]
    with pytest.raises(ValueError, match="pre-steps"):                                           # other extents
        radiomics.extract(small["scan"], small["mask"], DEV, classes=c["classes"], glszm=True, mesh=True, log_sigma=c["sigmas"], normalize={"scale": SCALE},
                          resample={"spacing": list(c["to"])}, buffers=res)
    plain = radiomics.extract(c["scan"], c["mask"], DEV)
    with pytest.raises(ValueError, match="pre-steps"):
        radiomics.extract(c["scan"], c["mask"], DEV, normalize=True, buffers=plain)


# ---- the command lines: one fresh process each -----------------------------------------------------------------------------------------------
def test_cli_extraction_tool_with_the_pre_steps_writes_the_rows_of_finish(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=13, mask_grid="own")      # scans at 0.9 x 0.9 x 3 mm
    loc = ["-m", "mmnn_sts_amd.radiomics", "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--modality", "t1"]
    out, bare = tmp_path / "radiomics.csv", tmp_path / "bare.csv"
    log = process(loc + ["--normalize", "--resample_spacing", "1,1,1", "--out", str(out)], tmp_path)
    assert "47 features" in log
    ds = ImageDataset(os.path.join(tree["image_loc"], "t1"), tree["key_loc"])
    radiomics.extract_tree(ds, DEV, bare)                                                        # without the flags: the same header
    cols, rows = radiomics.read_csv(out)
    assert cols == radiomics.read_csv(bare)[0] == ["MRN"] + list(radiomics.FEATURE_NAMES) and len(rows) == 3
    part = radiomics.extract_tree(ds, DEV, normalize=True, resample=(1, 1, 1))                   # one stacked read-back per batch
    differs = 0
    for k, p in enumerate(ds.patients):
        want = radiomics.finish(radiomics.extract(*ds._load(p), DEV, normalize=True, resample="1,1,1"))
        plain = radiomics.finish(radiomics.extract(*ds._load(p), DEV))
        row = next(r for r in rows if int(r[0]) == ds._uid_of(p))
        for n, v in want.items():
            assert float(row[cols.index(n)]) == v == part[k][n] or math.isnan(v), (p, n)
        differs += want["original_firstorder_Mean"] != plain["original_firstorder_Mean"]
    assert differs == 3


def test_cli_trains_on_the_normalised_resampled_table_then_infers_with_the_saved_scaler(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=6, seed=14, val_fraction=0.34)
    loc = ["--config", tiny_config(tmp_path), "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]
    out = tmp_path / "run"
    out.mkdir()
    main = os.path.join(ROOT, "main.py")
    log = process([main, "--output_path", str(out), "--radiomics", "--survival", "--image_loc", tree["image_loc"], "--normalize",
                    "--resample_spacing", "2,2,2", "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    for name in ("radiomics_features.csv", "radiomics_scaler.csv", "best_surv_model.pth"):
        assert (out / name).exists(), name
    cols, rows = radiomics.read_csv(out / "radiomics_features.csv")
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in radiomics.FEATURE_NAMES] and len(rows) == 6
    log = process([main, "--output_path", str(out), "--inference", "--radiomics", "--survival", "--weights", str(out / "best_surv_model.pth"),
                    "--rad_loc", str(out / "radiomics_features.csv"), *loc], out)
    assert "All C-indexes" in log
