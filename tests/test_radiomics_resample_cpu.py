"""The two pre-steps of the radiomics path without a device: the numpy restatement of the resampling (tests/_radiomics_resample_ref.py)
against scipy; the grid rule and the per-axis tables; the normalisation's restatement; the parser and both argument parsers; the column
names; the header, the binding and the size functions' refusals; and the bin counts of the device test's feature cases."""
import ctypes
import os

import numpy as np
import pytest

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_ref as R
from tests import _radiomics_resample_ref as P
from tests._radiomics_resample_cases import BIN_WIDTH, FEATURE_CASES, HORIZON, RESAMPLE_CASES, SCALE, affine_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCIPY_CASES = ("anisotropic_to_1mm", "to_2mm", "upsample_thin", "extent_1")
U = 2.0 ** -53


def _grid(c, origin=(0.0, 0.0, 0.0)):
    g = radiomics.resample_grid(c["scan"].shape, affine_of(c["spacing"], origin), c["to"])
    return g, radiomics.resample_tables(c["scan"].shape, g)


@pytest.mark.parametrize("name", SCIPY_CASES)
def test_restatement_against_scipy(name):
    """Coefficients against spline_filter, inside values against map_coordinates at c(j), order 3, mode 'mirror': within 2^-40 max|v|."""
    c = RESAMPLE_CASES[name]
    g, t = _grid(c)
    assert g.shape == c["out"]
    v = P.scaled(c["scan"], c["scale"])
    coef = P.prefilter(v, radiomics.resample_constants())
    val = P.evaluate(coef, g.shape, t)
    want_coef, want_val = P.by_scipy(v, g)
    inside, top = P.inside_of(g.shape, t), float(np.abs(v).max())
    e_coef, e_val = float(np.abs(coef - want_coef).max()), float(np.abs(val - want_val)[inside].max())
    print(name, "deviation / (2^-53 max|v|): coefficients", e_coef / top / U, "values", e_val / top / U)
    assert e_coef <= P.TOL * top and e_val <= P.TOL * top, (name, e_coef / top, e_val / top)
    out, mask = P.restate(c["scan"], c["mask"], g, t, radiomics.resample_constants(), c["scale"])
    assert out.dtype == np.float32 and mask.dtype == np.uint8 and out.shape == mask.shape == g.shape
    assert not out[~inside].any() and not mask[~inside].any() and np.array_equal(out[inside], val.astype(np.float32)[inside])


def test_constants():
    k = radiomics.resample_constants()
    z = k["pole"]
    assert z == np.sqrt(3.0) - 2.0 and k["gain"] == 6.0 and k["pole_gain"] == z / (z * z - 1.0)
    assert len(k["pole_power"]) == HORIZON == _lib.RESAMPLE_HORIZON and k["pole_power"][0] == 1.0 and k["pole_power"][1] == z
    assert abs(k["pole_power"][-1] * z) < 2.0 ** -53 * 2.0 ** -20       # what the horizon drops is far below fp64 resolution


def test_a_constant_volume_stays_constant_and_a_mask_moves_by_nearest_neighbour():
    g = radiomics.resample_grid((9, 8, 7), affine_of((0.8, 1.1, 5.0)), 1.0)
    t = radiomics.resample_tables((9, 8, 7), g)
    mask = np.zeros((9, 8, 7), np.uint8)
    mask[2:6, 3:5, 1:4] = 1
    out, m = P.restate(np.full((9, 8, 7), 130, np.int16), mask, g, t, radiomics.resample_constants())
    inside = P.inside_of(g.shape, t)
    assert np.abs(out[inside] - 130.0).max() <= 130.0 * 2.0 ** -23
    cx, cy, cz = P.coordinates(g)
    near = [np.clip(np.floor(c + 0.5), 0, n - 1).astype(int) for c, n in zip((cx, cy, cz), (9, 8, 7))]
    assert np.array_equal(m, mask[np.ix_(*near)] * inside) and m.sum() > 0
    nan_mask = mask.astype(np.float32)
    nan_mask[0, 0, 0] = np.nan
    assert P.restate(np.zeros((9, 8, 7), np.int16), nan_mask, g, t, radiomics.resample_constants())[1][0, 0, 0] == 1      # a NaN is not 0


def test_grid_rule():
    th = 0.3
    rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    A = np.eye(4)
    A[:3, :3] = rot @ np.diag([0.8, 1.1, 5.0])
    A[:3, 3] = (-40.0, 12.0, 3.0)
    shape = (13, 10, 9)
    g = radiomics.resample_grid(shape, A, (1, 1, 1))
    assert g.shape == (11, 11, 45) and not g.skip and g.ratio == pytest.approx((1.25, 1.0 / 1.1, 0.2), rel=1e-15)
    assert radiomics.spacing_of(g.affine) == pytest.approx((1.0, 1.0, 1.0), rel=1e-14)
    j = np.stack(np.meshgrid(*[np.arange(m) for m in g.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    c = (j + 0.5) * g.ratio - 0.5
    new, old = j @ g.affine[:3, :3].T + g.affine[:3, 3], c @ A[:3, :3].T + A[:3, 3]
    extent = float(np.linalg.norm(np.array(shape) * np.array([0.8, 1.1, 5.0])))
    assert np.abs(new - old).max() <= 1e-12 * extent
    kept = radiomics.resample_grid(shape, A, (1, 0, 0))                                      # an entry of 0 keeps its axis
    assert kept.shape == (11, 10, 9) and kept.ratio[1] == 1.0 and kept.ratio[2] == 1.0
    assert radiomics.spacing_of(kept.affine) == pytest.approx((1.0, 1.1, 5.0), rel=1e-14) and np.array_equal(kept.affine[:, 1:3], A[:, 1:3])
    for same in ((0, 0, 0), 0, (0.8, 1.1, 5.0)):
        noop = radiomics.resample_grid(shape, affine_of((0.8, 1.1, 5.0)), same)
        assert noop.skip and noop.shape == shape and np.array_equal(noop.affine, affine_of((0.8, 1.1, 5.0)))
    bare = radiomics.resample_grid((4, 4, 4), None, 0.5)                                     # without an affine: from the identity
    assert bare.shape == (8, 8, 8) and np.array_equal(bare.affine, np.array([[.5, 0, 0, -.25], [0, .5, 0, -.25], [0, 0, .5, -.25], [0, 0, 0, 1]]))
    assert radiomics.resample_grid((10, 10, 10), affine_of((1.1, 1.1, 1.1)), 1.0).shape == (11, 11, 11)   # 10 * 1.1 rounds above 11
    assert radiomics.resample_grid((3, 3, 3), affine_of((1, 1, 1)), 100.0).shape == (1, 1, 1)
    assert radiomics.resample_spacing(2) == (2.0, 2.0, 2.0) and radiomics.resample_spacing("1, 0,2") == (1.0, 0.0, 2.0)
    assert radiomics.resample_spacing({"spacing": [1, 1, 3]}) == (1.0, 1.0, 3.0) and radiomics.resample_spacing(None) is None


def test_the_last_x_plane_of_the_first_case_is_outside():
    c = RESAMPLE_CASES["anisotropic_to_1mm"]
    g, t = _grid(c)
    inside = P.inside_of(g.shape, t)
    assert int((~inside).sum()) == 495 and not inside[-1].any() and inside[:-1].all()
    assert g.shape[0] * g.ratio[0] - 13 > 0.5 * g.ratio[0]


def test_grid_errors_name_the_spacing():
    with pytest.raises(ConfigurationError, match="spacing.*2\\^31"):
        radiomics.resample_grid((512, 512, 48), affine_of((0.8, 0.8, 5.0)), 0.05)
    with pytest.raises(ConfigurationError, match="spacing.*2\\^31.*intermediate"):       # 200 x 3 x 3 out of 2 x 30000 x 30000: [z][y][mx] is too large
        radiomics.resample_grid((2, 30000, 30000), affine_of((1, 1, 1)), (0.01, 10000, 10000))
    assert _lib.lib().mmnn_resample_pair_workspace_bytes(2, 30000, 30000, 200, 3, 3) == -1
    for bad in (-1.0, float("nan"), float("inf"), (1, 1), (1, 2, 3, 4), "a,b,c", [True, 1, 1], {"spacings": 1}, {"spacing": [1, -1, 1]}, "", []):
        with pytest.raises(ConfigurationError, match="spacing"):
            radiomics.resample_grid((4, 4, 4), None, bad)
    with pytest.raises(ConfigurationError, match="spacing"):
        radiomics.resample_grid((4, 4, 4), np.diag([1.0, 0.0, 1.0, 1.0]), 1.0)


@pytest.mark.parametrize("name", list(RESAMPLE_CASES))
def test_tables(name):
    c = RESAMPLE_CASES[name]
    g, t = _grid(c)
    assert g.shape == c["out"] and t.dtype.itemsize == 56 == ctypes.sizeof(_lib.ResampleEntry) and len(t) == sum(g.shape)
    assert np.abs(t["w"].sum(axis=1) - 1.0).max() <= 4 * U and (t["w"] >= 0.0).all()
    for n, e, coords, r in zip(c["scan"].shape, P.split_tables(g.shape, t), P.coordinates(g), g.ratio):
        assert e["i"].min() >= 0 and e["i"].max() < n and e["nearest"].min() >= 0 and e["nearest"].max() < n
        assert np.array_equal(e["inside"] != 0, ~((coords < -0.5) | (coords >= n - 0.5)))
        f = np.floor(coords).astype(int)
        assert [[P.mirror(int(b) - 1 + k, n) for k in range(4)] for b in f] == e["i"].tolist()
        if n == 1:
            assert not e["i"].any() and not e["nearest"].any()
        if r == 1.0:                                          # a kept axis samples at the integers: t = 0
            assert np.array_equal(e["w"], np.tile([1.0 / 6.0, 2.0 / 3.0, 2.0 / 3.0 - 0.5, 0.0], (len(e), 1))) and e["inside"].all()


def test_mirror():
    assert [P.mirror(k, 4) for k in range(-3, 10)] == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3] and [P.mirror(k, 1) for k in (-2, 0, 5)] == [0, 0, 0]
    assert [P.mirror(k, 2) for k in range(-2, 5)] == [0, 1, 0, 1, 0, 1, 0]


def test_normalisation_restatement():
    rng = np.random.default_rng(5)
    v = rng.integers(-200, 1800, (7, 6, 5)).astype(np.int16)
    n, mean, sd = P.normalize_stats(v)
    assert n == 210 and mean == pytest.approx(v.astype(np.float64).mean(), rel=1e-15) and sd == pytest.approx(v.astype(np.float64).std(ddof=1), rel=1e-14)
    out = P.normalize(v, scale=100.0)
    assert out.dtype == np.float32 and abs(float(out.astype(np.float64).mean())) < 1e-4 and float(out.astype(np.float64).std(ddof=1)) == pytest.approx(100.0, rel=1e-6)
    clamped = P.normalize(v, scale=100.0, outliers=1.0)
    assert clamped.max() == 100.0 and clamped.min() == -100.0 and np.array_equal(clamped[np.abs(out) < 100.0], out[np.abs(out) < 100.0])
    assert np.isnan(P.normalize(np.full((3, 3, 3), 7, np.int16))).all()                         # a constant scan: 0 / 0
    bad = v.astype(np.float32)
    bad[1, 2, 3] = np.nan
    assert np.isnan(P.normalize(bad)).all() and np.isnan(P.normalize(bad, outliers=3.0)).all()
    bad[1, 2, 3] = np.inf
    assert np.isnan(P.normalize(bad)).all()
    assert np.array_equal(P.normalize(v, (-0.5, 100.0)), -P.normalize(v))                      # the z-score forgets an affine intensity map, up to its sign
    assert radiomics.normalize_settings(True) == (100.0, 0.0) and radiomics.normalize_settings({"outliers": 3}) == (100.0, 3.0)
    assert radiomics.normalize_settings(None) is None and radiomics.normalize_settings(False) is None and radiomics.normalize_settings((50, 2)) == (50.0, 2.0)
    for bad in ({"scale": 0}, {"scale": -1}, {"scale": float("inf")}, {"outliers": -1}, {"outliers": float("nan")}, {"scales": 1}, "yes", 3, {"scale": "x"},
                {"scale": True}):
        with pytest.raises(ConfigurationError, match="normalize"):
            radiomics.normalize_settings(bad)


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


def test_parser_accessors(tmp_path):
    off = _parser(tmp_path, None)
    assert off.radiomicsNormalize() is None and off.radiomicsResample() is None
    assert off.radiomicsNormalize(True) == (100.0, 0.0) and off.radiomicsNormalize(False, 50.0) == (50.0, 0.0) and off.radiomicsNormalize(False, None, 3.0) == (100.0, 3.0)
    assert off.radiomicsResample("1,1,1") == (1.0, 1.0, 1.0) and off.radiomicsResample("2") == (2.0, 2.0, 2.0)
    assert _parser(tmp_path, {"normalize": False}).radiomicsNormalize() is None and _parser(tmp_path, {"normalize": True}).radiomicsNormalize() == (100.0, 0.0)
    p = _parser(tmp_path, {"normalize": {"scale": 100, "outliers": 3}, "resample": {"spacing": [1, 1, 3]}})
    assert p.radiomicsNormalize() == (100.0, 3.0) and p.radiomicsResample() == (1.0, 1.0, 3.0)
    assert p.radiomicsNormalize(False, 10.0) == (10.0, 3.0) and p.radiomicsResample("2,2,0") == (2.0, 2.0, 0.0)     # a command line's values go first
    assert _parser(tmp_path, {"resample": {"spacing": 2}}).radiomicsResample() == (2.0, 2.0, 2.0)
    for bad in ({"normalize": "yes"}, {"normalize": 3}, {"normalize": {"scale": 0}}, {"normalize": {"outliers": -1}}, {"normalize": {"sd": 1}}, {"normalize": [100, 3]}):
        with pytest.raises(ConfigurationError, match="normalize"):
            _parser(tmp_path, bad).radiomicsNormalize()
    for bad in ({"resample": [1, 1, 1]}, {"resample": 1.0}, {"resample": {"spacing": [1, 1]}}, {"resample": {"spacing": [1, -1, 1]}}, {"resample": {"spacing": "1,1,1"}},
                {"resample": {"spacings": [1, 1, 1]}}, {"resample": {"spacing": [1, 1, "a"]}}, {"resample": {}}):
        with pytest.raises(ConfigurationError, match="spacing"):
            _parser(tmp_path, bad).radiomicsResample()
    with pytest.raises(ConfigurationError, match="normalize"):
        off.radiomicsNormalize(True, -5.0)
    with pytest.raises(ConfigurationError, match="spacing"):
        off.radiomicsResample("1,1")


def test_both_argument_parsers():
    import main
    tool = ["--image_loc", "a", "--key_loc", "b", "--out", "c"]
    for build, lead in ((radiomics.build_arg_parser, tool), (main.build_arg_parser, [])):
        a = build().parse_args(lead)
        assert (a.normalize, a.normalize_scale, a.normalize_outliers, a.resample_spacing) == (False, None, None, None)
        a = build().parse_args(lead + ["--normalize", "--normalize_scale", "50", "--normalize_outliers", "3", "--resample_spacing", "1,1,1"])
        assert (a.normalize, a.normalize_scale, a.normalize_outliers, a.resample_spacing) == (True, 50.0, 3.0, "1,1,1")
        for bad in (["--normalize_scale", "wide"], ["--normalize_outliers"], ["--resample_spacing"], ["--normalize", "1"]):
            with pytest.raises(SystemExit):
                build().parse_args(lead + bad)


def test_feature_names_do_not_depend_on_the_switches():
    import inspect
    assert "normalize" not in inspect.signature(radiomics.feature_names).parameters and "resample" not in inspect.signature(radiomics.feature_names).parameters
    tree = inspect.signature(radiomics.extract_tree).parameters      # (no switch of its own: `**switches` go to `extract` unchanged)
    for k in ("normalize", "resample"):
        assert inspect.signature(radiomics.extract).parameters[k].default is None and k not in tree
    assert tree["switches"].kind is inspect.Parameter.VAR_KEYWORD
    assert len(radiomics.feature_names()) == 47 and len(radiomics.feature_names("all", True, True, (1.0,))) == 106 + 92
    assert all(n.startswith(("original_", "log-sigma-")) for n in radiomics.feature_names("all", True, True, (1.0,)))


def test_header_binding_and_size_refusals():
    header = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    for word in ("int64_t mmnn_normalize_scan_workspace_bytes(int32_t x, int32_t y, int32_t z);", "} mmnn_normalize_desc;", "} mmnn_normalize_result;",
                 "int mmnn_normalize_scan(const mmnn_normalize_desc* d, const void* scan, float* out, mmnn_normalize_result* result, void* ws, void* stream);",
                 "int64_t mmnn_resample_pair_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t mx, int32_t my, int32_t mz);",
                 f"#define MMNN_RESAMPLE_HORIZON {_lib.RESAMPLE_HORIZON}", "} mmnn_resample_entry;", "} mmnn_resample_desc;", "**Parity with PyRadiomics is\n * unpinned**"):
        assert word in header, word
    assert ctypes.sizeof(_lib.NormalizeDesc) == 48 and _lib.NormalizeDesc.scale.offset == 32 and _lib.NORMALIZE_RESULT_BYTES == 32
    assert ctypes.sizeof(_lib.ResampleDesc) == 32 + 7 * 8 + 40 * 8 and _lib.ResampleDesc.pole.offset == 64 and _lib.ResampleDesc.pole_power.offset == 88
    assert [radiomics.RESAMPLE_ENTRY.fields[k][1] for k in ("w", "i", "nearest", "inside")] == [0, 32, 48, 52]
    assert os.path.exists(os.path.join(ROOT, "mmnn_sts_amd", "csrc", "radiomics_resample.hip"))
    L = _lib.lib()                                                                               # the size functions run on the host alone
    n = L.mmnn_normalize_scan_workspace_bytes
    assert n(0, 4, 4) == -1 and n(4, 4, -1) == -1 and n(2048, 1024, 1024) == -1 and n(13, 10, 9) > 0 and "2^31" in _lib.last_error()
    r = L.mmnn_resample_pair_workspace_bytes
    assert r(13, 10, 9, 11, 11, 45) >= 8 * (13 * 10 * 9 + 11 * 10 * 9 + 11 * 11 * 9)
    for bad in ((0, 4, 4, 4, 4, 4), (4, 4, 4, 4, 0, 4), (4, 4, -1, 4, 4, 4), (2048, 1024, 1024, 4, 4, 4), (4, 4, 4, 2048, 1024, 1024), (1, 1024, 1024, 4096, 1, 1)):
        assert r(*bad) == -1 and _lib.last_error(), bad
    with pytest.raises(ValueError, match="2\\^31"):
        radiomics.resample_workspace_bytes((4, 4, 4), (2048, 1024, 1024))


@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_feature_cases_set_no_flag(name):
    """On the restatement's output: no flag, 8 <= Ng <= 256 at the bin width, at least 16 ROI voxels; the same for the LoG image."""
    from tests import _radiomics_log_ref as LG
    c = FEATURE_CASES[name]
    g = radiomics.resample_grid(c["scan"].shape, affine_of(c["spacing"]), c["to"])
    scan, mask = P.restate(P.normalize(c["scan"], scale=SCALE), c["mask"], g, radiomics.resample_tables(c["scan"].shape, g), radiomics.resample_constants())
    ref = R.restate(scan, mask, BIN_WIDTH, 256, (1.0, 0.0), (1.0, 0.0))
    print(name, g.shape, "Ng", ref["n_bins"], "ROI", ref["n"])
    assert not (ref["empty"] or ref["nonfinite"] or ref["overflow"]) and 8 <= ref["n_bins"] <= 256 and ref["n"] >= 16 and ref["n"] == int(mask.sum())
    for s in c["sigmas"]:
        radius, taps, weight = radiomics.log_taps(s, radiomics.spacing_of(g.affine))
        sub = R.restate(LG.restate(scan, radius, taps, weight), mask, c["log_bin_width"], 256, (1.0, 0.0), (1.0, 0.0))
        print(name, "sigma", s, "Ng", sub["n_bins"])
        assert not (sub["empty"] or sub["nonfinite"] or sub["overflow"]) and 8 <= sub["n_bins"] <= 256
