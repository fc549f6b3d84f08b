"""The numpy restatement of the surface mesh (tests/_radiomics_mesh_ref.py) against its own invariants, hand values and the mpmath
evaluation; the library's triangle table and the generator against it; and the host side of `Radiomics: mesh_shape`: the names, the
derived features, the parser accessor, the flags, the header, the binding, the refusals of the C-ABI.  No GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_mesh_ref as M
from tests import _radiomics_ref as R
from tests._radiomics_mesh_cases import BOUND, FLAGGED, FROM_ZONES, MEASURED, MESH_CASES, MLP_STREAM, OBLIQUE, TILE, U, VERTICES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MS = {}


def _roi(name):
    c = MESH_CASES[name]
    return R.scaled(c["mask"], *c["mask_scale"]) != 0.0


def _ms(name):
    if name not in _MS:
        _MS[name] = M.restate(_roi(name), MESH_CASES[name]["L"], flagged=name in FLAGGED)
    return _MS[name]


def _config_roi(c):
    return np.array([[[c >> (x + 2 * y + 4 * z) & 1 for z in range(2)] for y in range(2)] for x in range(2)], dtype=bool)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def test_every_configuration_gives_a_balanced_mesh_of_positive_volume():
    tri, pts = M.table()
    assert tri[0, 15] == 0 and tri[255, 15] == 0 and int(tri[:, 15].max()) == 5
    for c in range(1, 256):
        assert 1 <= tri[c, 15] <= 5 or c == 255
        assert (tri[c, :3 * tri[c, 15]] >= 0).all() and (tri[c, 3 * tri[c, 15]:15] == -1).all() and (tri[c, :15] < 12).all()
        t = M.triangles(_config_roi(c))                      # the block alone in an empty volume: the padding closes it
        assert M.balanced(t) and M.volume48(t) > 0, c
    assert not M.balanced(M.triangles(_config_roi(1))[:-1])   # (the check does see an open mesh)


def test_random_masks_and_an_ellipsoid_give_a_balanced_mesh():
    rng = np.random.default_rng(99)
    for shape, p in (((7, 6, 5), 0.5), ((9, 4, 6), 0.2), ((5, 5, 5), 0.8), ((1, 8, 3), 0.5)):
        roi = rng.random(shape) < p
        ms = M.restate(roi)
        assert M.balanced(ms["triangles"]) and ms["volume48"] > 0
        assert ms["cfg"].sum() == np.prod([s + 1 for s in shape]) and ms["n_triangles"] == int((ms["cfg"] * M.table()[0][:, 15]).sum())
        # the table's vertices are the lattice crossings, each used
        assert np.array_equal(np.unique(ms["triangles"].reshape(-1, 3), axis=0), np.unique(ms["vertices"], axis=0))
    ms = _ms("ellipsoid_24")
    assert M.balanced(ms["triangles"]) and 0 < ms["volume48"] / 48.0 < _roi("ellipsoid_24").sum()


def test_library_table_equals_the_restatement():
    got, (tri, _), (l48, nsum) = radiomics.mesh_table(), M.table(), M.shortcut_tables()
    assert got["tri"].shape == (256, 16) and np.array_equal(got["tri"], tri)
    assert np.array_equal(got["l48"], l48) and np.array_equal(got["nsum"], nsum)
    assert np.abs(nsum).max() <= 127                          # the cell pass packs the normals into signed bytes


def test_committed_header_is_what_the_generator_writes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mesh_table
    finally:
        sys.path.pop(0)
    assert open(os.path.join(ROOT, "mmnn_sts_amd", "csrc", "mesh_table.hpp")).read() == gen_mesh_table.render()
    tri, l48, nsum = gen_mesh_table.table()
    assert np.array_equal(np.array(tri, dtype=np.int8), M.table()[0]) and np.array_equal(np.array(l48), M.shortcut_tables()[0])


def test_single_voxel_by_hand():
    for name in ("voxel_1x1x1", "single_voxel"):
        ms = _ms(name)
        assert (ms["n_vertices"], ms["n_triangles"], ms["volume48"]) == (6, 8, 8)
        assert ms["area"] == pytest.approx(math.sqrt(3.0), rel=4 * U) and ms["q"].tolist() == [4.0, 4.0, 4.0, 4.0]
        f = radiomics.mesh_features({"volume48": 8, "area": ms["area"], "q": ms["q"]}, np.eye(3))
        assert f["MeshVolume"] == pytest.approx(1.0 / 6.0, rel=2 * U)
        assert [f[k] for k in M.MESH_SHAPE[4:]] == [1.0, 1.0, 1.0, 1.0]
    assert _ms("voxel_1x1x1")["cfg"][[1, 2, 4, 8, 16, 32, 64, 128]].tolist() == [1] * 8 and _ms("voxel_1x1x1")["cfg"].sum() == 8


def test_hand_values_of_the_small_shapes():
    full = _ms("full_3x2x4")
    assert full["cfg"].sum() == 4 * 3 * 5 and full["cfg"][0] == 0 and full["cfg"][255] == 2 * 1 * 3
    # a box of a x b x c voxels: its faces are cut at half a voxel, the 8 corners and 12 edges are bevelled
    assert full["n_vertices"] == 2 * (3 * 2 + 2 * 4 + 3 * 4) == VERTICES["full_3x2x4"]
    assert full["q"][0] == 4.0 * ((3 - 1) ** 2 + (2 - 1) ** 2 + 4 ** 2)      # between the two z faces (the longest axis), corner voxel to corner voxel
    line = _ms("line_1x1x300")
    assert line["n_vertices"] == 2 + 4 * 300 and line["q"][0] == 600.0 ** 2 and line["q"][1] == 4.0 and line["q"][2] == line["q"][3] == 600.0 ** 2
    wrap = _ms("row_wrap")
    assert (wrap["n_vertices"], wrap["n_triangles"], wrap["volume48"]) == (24, 32, 32)        # four separate voxels: nothing joins across a row end
    assert wrap["area"] == pytest.approx(4 * math.sqrt(3.0), rel=8 * U)
    both = _ms("all_configs")
    assert (both["cfg"][1:255] >= 1).all() and both["n_vertices"] % TILE == 0
    for name, n in VERTICES.items():
        assert _ms(name)["n_vertices"] == n, name
    ell = _ms("ellipsoid_24")
    assert ell["n_vertices"] > 2 * TILE and ell["n_vertices"] % TILE not in (0, 1)
    assert all(_ms(k)["n_vertices"] % 2 == 0 for k in MESH_CASES if k not in FLAGGED)       # why no case has 256 k + 1 vertices
    for p in ("plate_x", "plate_y", "plate_z"):
        assert len(set(_ms(p)["q"][1:].tolist())) == 3 and len(set(_ms(p + "_oblique")["q"][1:].tolist())) == 3, p
    # a plate one voxel thick along x: fixing x leaves the whole plate, so Row is the 3-D diameter
    assert _ms("plate_x")["q"][3] == _ms("plate_x")["q"][0] and _ms("plate_y")["q"][2] == _ms("plate_y")["q"][0]
    assert _ms("plate_z")["q"][1] == _ms("plate_z")["q"][0]


@pytest.mark.parametrize("name", [n for n in MESH_CASES if n not in FLAGGED])
def test_shortcut_equals_the_triangle_sums(name):
    ms, roi = _ms(name), _roi(name)
    l48, nsum = M.shortcut_tables()
    cfg = M.configurations(roi)
    lo = np.argwhere(roi).min(axis=0)
    o = np.argwhere(cfg >= 0).astype(np.int64) - 1 - lo                   # every cell's origin, relative to the bounding box
    c = cfg.ravel()
    assert int(l48[c].sum() + 2 * (o * nsum[c]).sum()) == ms["volume48"]
    assert int((o * 0 + nsum[c]).sum()) == 0                              # closed: the normals cancel, so the origin does not matter
    t = ms["triangles"]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).astype(np.float64)
    tri_area = float((np.linalg.norm(n @ M.cofactor(ms["L"]).T, axis=1) / 8.0).sum())
    assert ms["area"] == pytest.approx(tri_area, rel=1e-13)
    assert len(ms["vertices"]) == len(np.unique(t.reshape(-1, 3), axis=0))
    own = M.area_deviation(ms["area"], ms["cfg"], ms["L"])
    assert own <= MEASURED, (name, own / U)


def test_tolerance_and_cases():
    assert BOUND == 64 * U and 8 * MEASURED < BOUND
    assert all(MESH_CASES[k]["L"] is None for k in FROM_ZONES) and set(FLAGGED) <= set(FROM_ZONES)
    assert {"voxel_1x1x1", "full_3x2x4", "all_configs", "row_wrap", "line_1x1x300", "plate_x", "plate_y", "plate_z", "ellipsoid_24", "box_v258",
            "box_v256", "ellipsoid_24_oblique", "plate_x_oblique", "plate_y_oblique", "plate_z_oblique"} <= set(MESH_CASES)
    assert np.linalg.det(OBLIQUE) < 0 and MESH_CASES["ellipsoid_24_oblique"]["L"] is OBLIQUE
    for k in FLAGGED:
        ms = _ms(k)
        assert not ms["cfg"].any() and (ms["n_vertices"], ms["n_triangles"], ms["volume48"]) == (0, 0, 0)
        assert math.isnan(ms["area"]) and np.isnan(ms["q"]).all()
    # an orthogonal map leaves the diameters alone and the area too
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    a, b = _ms("ellipsoid_24"), M.restate(_roi("ellipsoid_24"), rot)
    assert a["q"].tolist() == b["q"].tolist() and a["area"] == pytest.approx(b["area"], rel=64 * U)
    # scaling by 2 scales areas by 4 and squared diameters by 4
    c = M.restate(_roi("ellipsoid_24"), 2.0 * np.eye(3))
    assert c["q"].tolist() == (4.0 * a["q"]).tolist() and c["area"] == 4.0 * a["area"]


# ---- derived features, names, parser, header, binding ----------------------------------------------------------------------------------------
def test_derived_features():
    ms = _ms("ellipsoid_24_oblique")
    mesh = {"volume48": ms["volume48"], "area": ms["area"], "q": ms["q"]}
    got, want = radiomics.mesh_features(mesh, OBLIQUE), M.derived(ms["volume48"], ms["area"], ms["q"], OBLIQUE)
    assert list(got) == list(M.MESH_SHAPE) == list(radiomics.MESH_SHAPE)
    for k in M.MESH_SHAPE:
        assert got[k] == pytest.approx(want[k], rel=8 * U), k
    V = ms["volume48"] / 48.0 * abs(np.linalg.det(OBLIQUE))
    assert got["MeshVolume"] == pytest.approx(V, rel=4 * U) and got["SurfaceVolumeRatio"] == pytest.approx(ms["area"] / V, rel=4 * U)
    assert 0.0 < got["Sphericity"] < 1.0 and got["Maximum3DDiameter"] == math.sqrt(ms["q"][0]) / 2.0
    assert got["Maximum3DDiameter"] >= max(got[k] for k in M.MESH_SHAPE[5:])
    # a ball of radius r in voxels: the mesh volume and area tend to the sphere's, sphericity towards 1 from below (a voxel surface is rough)
    g = np.indices((31, 31, 31)) - 15
    ball = M.restate((g ** 2).sum(axis=0) <= 12.5 ** 2)
    f = radiomics.mesh_features({"volume48": ball["volume48"], "area": ball["area"], "q": ball["q"]}, np.eye(3))
    assert f["MeshVolume"] == pytest.approx(4.0 / 3.0 * math.pi * 12.5 ** 3, rel=0.02) and 0.85 < f["Sphericity"] < 1.0
    assert f["Maximum3DDiameter"] == pytest.approx(25.0, abs=1.5)
    # through features_of, behind every other column
    fields = {"empty": False, "nonfinite": False, "overflow": False, "n": 7, "n_bins": 1, "moments": [21, 21, 21, 91, 91, 91, 63, 63, 63],
              "firstorder": np.arange(17.0), "glcm": np.arange(23.0)}
    out = radiomics.features_of(fields, None, mesh=mesh)
    assert list(out) == list(radiomics.feature_names(mesh=True)) and out["original_shape_SurfaceArea"] == ms["area"]
    assert list(radiomics.features_of(fields, None)) == list(radiomics.FEATURE_NAMES)
    with pytest.raises(ConfigurationError, match="no voxel"):
        radiomics.features_of(dict(fields, empty=True), None, mesh=mesh)


def test_finish_refuses_another_affine_than_the_one_enqueued():
    ms = _ms("plate_x")
    raw = np.zeros(_lib.RADIOMICS_RESULT_BYTES + _lib.RADIOMICS_MESH_BYTES, dtype=np.uint8)
    head = raw[:_lib.RADIOMICS_RESULT_INT64 * 8].view(np.int64)
    head[0], head[7:16], head[16] = 7, [21, 21, 21, 91, 91, 91, 63, 63, 63], 1
    tail = raw[_lib.RADIOMICS_RESULT_BYTES:]
    tail[:24].view(np.int64)[:] = [ms["n_vertices"], ms["n_triangles"], ms["volume48"]]
    tail[24:].view(np.float64)[:] = [ms["area"], *ms["q"]]
    got = radiomics.unpack_mesh(tail)
    assert [got[k] for k in M.INTEGERS] == [ms[k] for k in M.INTEGERS] and got["area"] == ms["area"] and got["q"].tolist() == ms["q"].tolist()
    r = radiomics.RadiomicsResult(None, None, None, None, (9, 8, 7), None, 25.0, 256, mesh_shape=True, linear=np.eye(3))
    out = radiomics._features_of_stacked(raw, r, None, "t")
    assert out["original_shape_Maximum2DDiameterRow"] == math.sqrt(ms["q"][3]) / 2.0 and len(out) == 55
    assert radiomics._features_of_stacked(raw, r, np.eye(4), "t") == out
    aff = np.eye(4)
    aff[:3, :3] = OBLIQUE
    with pytest.raises(ValueError, match="enqueued under"):
        radiomics._features_of_stacked(raw, r, aff, "t")
    r.linear = OBLIQUE.copy()
    assert radiomics._features_of_stacked(raw, r, aff, "t")["original_shape_MeshVolume"] == pytest.approx(
        ms["volume48"] / 48.0 * abs(np.linalg.det(OBLIQUE)), rel=4 * U)
    with pytest.raises(ValueError, match="enqueued under"):
        radiomics._features_of_stacked(raw, r, None, "t")


def test_feature_names():
    names = tuple(f"original_shape_{n}" for n in M.MESH_SHAPE)
    assert names == ("original_shape_MeshVolume", "original_shape_SurfaceArea", "original_shape_SurfaceVolumeRatio", "original_shape_Sphericity",
                     "original_shape_Maximum3DDiameter", "original_shape_Maximum2DDiameterSlice", "original_shape_Maximum2DDiameterColumn",
                     "original_shape_Maximum2DDiameterRow")
    for classes in ((), ["glrlm"], "all"):
        for glszm in (False, True):
            plain, wide = radiomics.feature_names(classes, glszm), radiomics.feature_names(classes, glszm, mesh=True)
            assert radiomics.feature_names(classes, glszm, mesh=False) == plain and wide == plain + names
    assert radiomics.feature_names() == radiomics.FEATURE_NAMES and len(radiomics.FEATURE_NAMES) == 47
    assert len(radiomics.feature_names(mesh=True)) == 55 and len(radiomics.feature_names("all", True, True)) == 106
    assert len(set(radiomics.feature_names("all", True, True))) == 106 and len(radiomics.feature_names("all", True)) == 98
    assert radiomics.SHAPE == ("VoxelVolume", "MajorAxisLength", "MinorAxisLength", "LeastAxisLength", "Elongation", "Flatness")


def test_binding_constants():
    assert _lib.RADIOMICS_MESH_BYTES == 64 and _lib.RADIOMICS_MESH_CONFIGS == 256 and _lib.RADIOMICS_MESH_TRI_ROW == 16
    fields = {f.name for f in radiomics.RadiomicsResult.__dataclass_fields__.values()}
    assert {"mesh", "mesh_cfg", "mesh_workspace", "linear", "mesh_shape"} <= fields
    import inspect
    assert inspect.signature(radiomics.extract).parameters["mesh"].default is False
    # (`extract_tree` states no switch of its own: it hands `**switches` to `extract`, whose default this then is)
    tree = inspect.signature(radiomics.extract_tree).parameters
    assert "mesh" not in tree and tree["switches"].kind is inspect.Parameter.VAR_KEYWORD


def _parser(tmp_path, rad):
    import yaml
    from mmnn_sts_amd.parser.parser import Parser
    cfg = {"ImageModel": {"name": "tinydensenet", "modality": "t1t2", "feature_layers": 12, "num_classes": 2, "spatial_dims": 3, "in_channels": 2,
                          "dropout_prob": 0.2},
           "ClinicalModel": {"NUM_PREDICTORS": 32, "PRE_OP_PREDICTORS": [], "POST_OP_PREDICTORS": []}, "Hyperparameters": {"train_batch_size": 2}}
    if rad is not None:
        cfg["Radiomics"] = rad
    (tmp_path / "c.yaml").write_text(yaml.safe_dump(cfg))
    p = Parser(str(tmp_path / "c.yaml"))
    p.parseConfig()
    return p


def test_parser_accessor_and_flags(tmp_path):
    assert _parser(tmp_path, None).radiomicsMesh() is False
    assert _parser(tmp_path, {"glszm": True}).radiomicsMesh() is False
    assert _parser(tmp_path, {"mesh_shape": False}).radiomicsMesh() is False
    p = _parser(tmp_path, {"bin_width": 10, "max_bins": 128, "classes": ["ngtdm"], "glszm": True, "mesh_shape": True})
    assert p.radiomicsMesh() is True and p.radiomicsZones() is True and p.radiomicsClasses() == ("ngtdm",)
    assert p.radiomicsConfig() == {"bin_width": 10.0, "max_bins": 128, "standardize": True}          # exactly its three keys
    for bad in ("yes", 1, ["mesh_shape"], None):
        with pytest.raises(ConfigurationError, match="mesh_shape"):
            _parser(tmp_path, {"mesh_shape": bad}).radiomicsMesh()
    sys.path.insert(0, ROOT)
    try:
        import main
    finally:
        sys.path.pop(0)
    assert main.build_arg_parser().parse_args(["--radiomics", "--mesh_shape"]).mesh_shape is True
    assert main.build_arg_parser().parse_args(["--radiomics"]).mesh_shape is False
    with pytest.raises(SystemExit):
        radiomics.main(["--mesh_shape"])                                                             # (the required locations are missing)
    with pytest.raises(SystemExit):
        radiomics.main(["--image_loc", "a", "--key_loc", "b", "--out", "c", "--mesh_shape=1"])      # a switch takes no value


def test_header_declares_the_mesh_call():
    header = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    for word in ("int64_t mmnn_radiomics_mesh_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins);",
                 "int mmnn_radiomics_mesh(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws, const double* linear,",
                 "mmnn_radiomics_mesh_result* out, uint64_t* cfg, void* ws4, void* stream);",
                 "int mmnn_radiomics_mesh_table(int8_t* tri, int32_t* l48, int32_t* nsum);", "} mmnn_radiomics_mesh_result;",
                 "Slice holds z fixed, Column y, Row x"):
        assert word in header, word
    for name in M.INTEGERS + ("area", "q[4]", "cfg"):
        assert name in header, name


def test_refusals_without_a_device():
    """Every refusal is made before any launch, so none of these calls touches a device: the pointers are never followed."""
    L = _lib.lib()
    assert L.mmnn_radiomics_mesh_workspace_bytes(0, 4, 4, 256) == -1 and L.mmnn_radiomics_mesh_workspace_bytes(4, 4, -1, 256) == -1
    assert L.mmnn_radiomics_mesh_workspace_bytes(4, 4, 4, 0) == -1
    assert L.mmnn_radiomics_mesh_workspace_bytes(4, 4, 4, _lib.RADIOMICS_MAX_BINS + 1) == -1
    assert L.mmnn_radiomics_mesh_workspace_bytes(2048, 2048, 512, 256) == -1 and "2^31" in _lib.last_error()
    assert L.mmnn_radiomics_mesh_workspace_bytes(4, 4, 4, 16) == 256 + 3 * ((3 * 125 * 4 + 255) // 256 * 256)
    assert L.mmnn_radiomics_mesh_workspace_bytes(1, 1, 2 ** 31 - 1, 16) > 3 * 3 * 4 * 4 * 2 ** 31        # the sizes are 64-bit
    good = dict(x=4, y=4, z=4, scan_type=4, mask_type=2, scan_slope=1.0, scan_inter=0.0, mask_slope=1.0, mask_inter=0.0, bin_width=25.0, max_bins=16)
    lin = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    p = 1 << 20                                                # result, ws, [linear], out, cfg, ws4: aligned, never followed
    ptrs = [p, p + 65536, p + 1024, p + 2048, p + 32768]
    call = lambda desc, q, linear=lin: L.mmnn_radiomics_mesh(desc, q[0], q[1], linear, q[2], q[3], q[4], None)
    for bad in (dict(bin_width=0.0), dict(bin_width=float("nan")), dict(scan_type=3), dict(mask_type=1), dict(x=0), dict(max_bins=0),
                dict(max_bins=_lib.RADIOMICS_MAX_BINS + 1)):
        assert call(ctypes.byref(_lib.RadiomicsDesc(**dict(good, **bad))), ptrs) == 1 and _lib.last_error(), bad
    desc = ctypes.byref(_lib.RadiomicsDesc(**good))
    assert call(None, ptrs) == 1 and "null" in _lib.last_error()
    assert call(desc, ptrs, None) == 1 and "null" in _lib.last_error()
    for k in range(len(ptrs)):
        assert call(desc, [None if q == k else v for q, v in enumerate(ptrs)]) == 1 and "null" in _lib.last_error(), k
    for k, step in ((0, 4), (1, 64), (2, 4), (3, 4), (4, 64)):
        assert call(desc, [v + step if q == k else v for q, v in enumerate(ptrs)]) == 1 and "misaligned" in _lib.last_error(), k
    for k, v in ((0, float("nan")), (4, float("inf")), (8, float("-inf"))):
        vals = [1.0, 0, 0, 0, 1, 0, 0, 0, 1]
        vals[k] = v
        assert call(desc, ptrs, (ctypes.c_double * 9)(*vals)) == 1 and f"linear[{k}]" in _lib.last_error()
    assert L.mmnn_radiomics_mesh_table(None, None, None) == 1 and "null" in _lib.last_error()


@pytest.mark.parametrize("width", sorted(MLP_STREAM))
def test_mlp_input_stream_is_the_first_well_conditioned_one(width):
    """The rule beside MLP_STREAM of tests/_radiomics_texture_cases.py, as tests/test_radiomics_zones_cpu.py asserts it for its widths."""
    import torch
    from oracle import restatement as OR
    from tests import test_tail_ops_gpu as TT
    from tests._util import synth_sd
    sd = synth_sd(OR.mlp_schema(width, 2, 12), f"radmlp{width}.")
    cot = TT._u(f"rad/mlp/cot/{width}", (4, 12))

    def fits(k):
        x = TT._u(f"rad/mlp/x/{width}/{k}", (4, width))
        ref, leaves, pres = TT.mlp_ref(sd, x, True)
        if min(float(p.detach().abs().min()) for p in pres) < TT.RELU_MARGIN:
            return False
        (ref * cot.double()).sum().backward()
        r32, l32, _ = TT.mlp_ref(sd, x, True, dtype=torch.float32)
        (r32 * cot).sum().backward()
        errs = [TT.rel_err(r32.detach().numpy(), ref.detach().numpy()), TT.rel_err(l32["x"].grad.numpy(), leaves["x"].grad.numpy())]
        errs += [TT.mlp_grad_err(k_, l32[k_].grad, leaves, True) for k_ in TT.MLP_PARAM_KEYS]
        return max(errs) <= TT.BAR / 4

    assert [fits(k) for k in range(MLP_STREAM[width] + 1)] == [False] * MLP_STREAM[width] + [True]
