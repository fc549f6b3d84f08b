"""The Laplacian-of-Gaussian image type without a device: the numpy restatement of the filter (tests/_radiomics_log_ref.py) against scipy,
an impulse and a constant; `log_taps`; the column names and counts; the parser's `Radiomics: log`; the header; and the bin counts of the
device test's feature cases."""
import os

import numpy as np
import pytest

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_log_ref as L
from tests import _radiomics_ref as R
from tests._radiomics_log_cases import FEATURE_CASES, FILTER_CASES, MLP_STREAM, affine_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _taps(c):
    return radiomics.log_taps(c["sigma"], c["spacing"])


@pytest.mark.parametrize("name", list(FILTER_CASES))
def test_restatement_against_scipy(name):
    """Per axis scipy's gaussian_filter of order 2, corrected by -d.sum() x order 0, weighted and summed: within 2^-40 S."""
    c = FILTER_CASES[name]
    radius, taps, weight = _taps(c)
    assert tuple(radius) == c["radii"]
    v = L.scaled(c["scan"], c["scale"])
    S = L.scale_S(v, radius, taps, weight)
    own = L.restate(c["scan"], radius, taps, weight, c["scale"], rounded=False)
    err = float(np.abs(own - L.by_scipy(v, c["sigma"], c["spacing"])).max())
    print(name, "deviation / S", err / S)
    assert err <= L.TOL * S, (name, err / S)
    assert L.restate(c["scan"], radius, taps, weight, c["scale"]).dtype == np.float32


def test_scaling_rule():
    raw = np.array([[[-3, 7]]], dtype=np.int16)
    assert np.array_equal(L.scaled(raw, (0.0, 5.0)), [[[-3.0, 7.0]]]) and np.array_equal(L.scaled(raw, (-0.5, 100.0)), [[[101.5, 96.5]]])


@pytest.mark.parametrize("sigma,spacing", [(1.0, (0.8, 1.1, 5.0)), (2.0, (1.0, 1.0, 1.0))])
def test_impulse_gives_the_outer_products_of_the_taps(sigma, spacing):
    radius, taps, weight = radiomics.log_taps(sigma, spacing)
    (gx, hx), (gy, hy), (gz, hz) = L.split_taps(radius, taps)
    shape = tuple(2 * int(r) + 1 for r in radius)
    v = np.zeros(shape)
    v[tuple(int(r) for r in radius)] = 1.0
    out = L.restate(v, radius, taps, weight, rounded=False)
    # out(p) = sum_t w[t] v(p + t): the impulse at the centre puts tap t at p = centre - t, i.e. the reversed taps (which are symmetric)
    o = lambda a, b, c: a[::-1, None, None] * b[None, ::-1, None] * c[None, None, ::-1]
    want = gz[None, None, ::-1] * ((gy[None, ::-1, None] * hx[::-1, None, None]) * weight[0] + (hy[None, ::-1, None] * gx[::-1, None, None]) * weight[1]) \
        + (hz[None, None, ::-1] * (gy[None, ::-1, None] * gx[::-1, None, None])) * weight[2]
    assert np.array_equal(out, want)
    plain = weight[0] * o(hx, gy, gz) + weight[1] * o(gx, hy, gz) + weight[2] * o(gx, gy, hz)
    assert np.allclose(out, plain, rtol=0.0, atol=2.0 ** -48 * np.abs(plain).max())
    assert out[tuple(int(r) for r in radius)] < 0.0            # the centre of a LoG of a bright blob is negative


@pytest.mark.parametrize("name", ["radii_at_extent", "small_radii", "radius_above_extents", "larger_radii", "radius_64"])
def test_constant_volume_filters_to_zero(name):
    c = FILTER_CASES[name]
    radius, taps, weight = _taps(c)
    v = np.full(c["scan"].shape, 1234.0)
    out = L.restate(v, radius, taps, weight, rounded=False)
    assert float(np.abs(out).max()) <= L.TOL * L.scale_S(v, radius, taps, weight)


def test_log_taps():
    for sigma, spacing, radii in [(3.0, (0.8, 1.1, 5.0), (15, 11, 2)), (1.0, (0.8, 1.1, 5.0), (5, 4, 1)), (2.0, (1, 1, 1), (8, 8, 8)),
                                  (5.0, (0.9, 0.9, 2.5), (22, 22, 8)), (16.0, (1, 1, 1), (64, 64, 64)), (8.0, (0.5, 0.5, 0.5), (64, 64, 64))]:
        radius, taps, weight = radiomics.log_taps(sigma, spacing)
        assert tuple(radius) == radii and taps.dtype == np.float64 and taps.size == sum(2 * (2 * r + 1) for r in radii)
        for (g, h), r, s, w in zip(L.split_taps(radius, taps), radii, spacing, weight):
            assert g.size == h.size == 2 * r + 1 and abs(g.sum() - 1.0) <= 2.0 ** -50 and abs(h.sum()) <= L.TOL * np.abs(h).sum()     # (what a constant volume is held to)
            assert np.array_equal(g, g[::-1]) and np.array_equal(h, h[::-1]) and h[r] < 0.0 and (g > 0.0).all()
            assert w == sigma * sigma / (s * s)
    assert _lib.LOG_FILTER_MAX_RADIUS >= 64
    with pytest.raises(ConfigurationError, match=r"0\.4.*z axis.*5\.0"):
        radiomics.log_taps(0.4, (0.8, 0.8, 5.0))                 # 0.08 voxels along z: radius 0
    with pytest.raises(ConfigurationError, match=r"30\.0.*x axis.*0\.5"):
        radiomics.log_taps(30.0, (0.5, 1.0, 1.0))                # 60 voxels along x: radius 240
    assert tuple(radiomics.log_taps((_lib.LOG_FILTER_MAX_RADIUS + 0.25) / 4.0)[0]) == (_lib.LOG_FILTER_MAX_RADIUS,) * 3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ConfigurationError):
            radiomics.log_taps(bad)


def test_spacing_is_the_column_norms_of_the_linear_part():
    assert radiomics.spacing_of(None) == (1.0, 1.0, 1.0)
    assert radiomics.spacing_of(affine_of((0.8, 1.1, 5.0))) == (0.8, 1.1, 5.0)
    th = 0.3
    rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    aff = np.eye(4)
    aff[:3, :3] = rot @ np.diag([0.8, 1.1, 5.0])
    aff[:3, 3] = (-40.0, 12.0, 3.0)
    assert radiomics.spacing_of(aff) == pytest.approx((0.8, 1.1, 5.0), rel=1e-15)


def test_feature_names():
    assert radiomics.feature_names() == radiomics.FEATURE_NAMES and radiomics.feature_names(log_sigma=()) == radiomics.FEATURE_NAMES
    assert radiomics.feature_names("all", True, True) == radiomics.feature_names("all", True, True, ()) and len(radiomics.feature_names("all", True, True)) == 106
    assert radiomics.log_image_type(3) == "log-sigma-3-0-mm-3D" and radiomics.log_image_type(1.5) == "log-sigma-1-5-mm-3D"
    one = radiomics.feature_names(log_sigma=(3,))
    assert len(one) == 47 + 41 and one[:47] == radiomics.FEATURE_NAMES and one[47] == "log-sigma-3-0-mm-3D_firstorder_Energy"
    assert one[47 + 17] == "log-sigma-3-0-mm-3D_firstorder_TotalEnergy" and one[47 + 18] == "log-sigma-3-0-mm-3D_glcm_Autocorrelation"
    assert one[-1] == "log-sigma-3-0-mm-3D_glcm_SumSquares" and not any("shape" in n for n in one[47:])
    two = radiomics.feature_names(log_sigma=(3, 1.0, 3.0))                       # de-duplicated, ascending
    assert len(two) == 47 + 41 * 2 and two[47].startswith("log-sigma-1-0-mm-3D_") and two[88].startswith("log-sigma-3-0-mm-3D_") and len(set(two)) == len(two)
    assert radiomics.feature_names(log_sigma="1,3") == two
    every = radiomics.feature_names("all", True, True, (1.5,))
    assert len(every) == 106 + 92 and every[:106] == radiomics.feature_names("all", True, True) and not any("shape" in n for n in every[106:])
    assert [n.split("_")[1] for n in every[106:]] == ["firstorder"] * 18 + ["glcm"] * 23 + ["glrlm"] * 16 + ["gldm"] * 14 + ["ngtdm"] * 5 + ["glszm"] * 16
    assert len(radiomics.feature_names(["gldm"], False, True, (1, 2, 3))) == 47 + 14 + 8 + 3 * (41 + 14)
    for bad in ([0.0], [-1], ["x"], [float("nan")], [float("inf")], [True], {"a": 1}):
        with pytest.raises(ConfigurationError, match="positive finite"):
            radiomics.log_sigmas(bad)
    assert radiomics.log_sigmas(None) == () and radiomics.log_sigmas(2) == (2.0,) and radiomics.log_sigmas("3, 1") == (1.0, 3.0)


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


def test_parser_accessor(tmp_path):
    assert _parser(tmp_path, None).radiomicsLog() == {"sigma": (), "bin_width": 25.0}
    assert _parser(tmp_path, {"bin_width": 10}).radiomicsLog() == {"sigma": (), "bin_width": 10.0}
    assert _parser(tmp_path, {"bin_width": 10, "log": {"sigma": [3.0, 1, 3]}}).radiomicsLog() == {"sigma": (1.0, 3.0), "bin_width": 10.0}
    p = _parser(tmp_path, {"log": {"sigma": [1.0, 3.0], "bin_width": 5}})
    assert p.radiomicsLog() == {"sigma": (1.0, 3.0), "bin_width": 5.0}
    assert p.radiomicsLog("2", 7.5) == {"sigma": (2.0,), "bin_width": 7.5}          # a command line's values go first
    assert p.radiomicsConfig()["bin_width"] == 25.0
    for bad in ({"log": [1.0]}, {"log": {"sigma": 1.0}}, {"log": {"sigma": [0.0]}}, {"log": {"sigma": [1.0, "a"]}}, {"log": {"sigma": [float("inf")]}},
                {"log": {"sigma": [1.0], "bin_width": 0}}, {"log": {"sigma": [1.0], "bin_width": "wide"}}, {"log": {"sigmas": [1.0]}}):
        with pytest.raises(ConfigurationError, match="sigma|positive finite"):
            _parser(tmp_path, bad).radiomicsLog()


def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    for word in ("int64_t mmnn_log_filter_workspace_bytes(int32_t x, int32_t y, int32_t z);",
                 "int mmnn_log_filter(const mmnn_log_filter_desc* d, const void* scan, const double* taps, float* out, void* ws, void* stream);",
                 f"#define MMNN_LOG_FILTER_MAX_RADIUS {_lib.LOG_FILTER_MAX_RADIUS}", "} mmnn_log_filter_desc;"):
        assert word in header, word
    import ctypes
    assert ctypes.sizeof(_lib.LogFilterDesc) == 72 and _lib.LogFilterDesc.radius.offset == 32 and _lib.LogFilterDesc.weight.offset == 48
    assert os.path.exists(os.path.join(ROOT, "mmnn_sts_amd", "csrc", "radiomics_filter.hip"))


@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_feature_cases_stay_clear_of_the_overflow_flag(name):
    c = FEATURE_CASES[name]
    for s in c["sigmas"]:
        radius, taps, weight = radiomics.log_taps(s, c["spacing"])
        ref = R.restate(L.restate(c["scan"], radius, taps, weight), c["mask"], c["bin_width"], 256, (1.0, 0.0), (1.0, 0.0))
        print(name, s, "Ng", ref["n_bins"])
        assert 8 <= ref["n_bins"] <= 256 and not (ref["empty"] or ref["nonfinite"] or ref["overflow"]), (name, s, ref["n_bins"])


@pytest.mark.parametrize("width", sorted(MLP_STREAM))
def test_mlp_input_stream_is_the_first_well_conditioned_one(width):
    """The rule beside MLP_STREAM: off the ReLU branch points, and torch's own fp32 evaluation within a quarter of the bar of the fp64 one."""
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
