"""The numpy restatement of the texture classes (tests/_radiomics_texture_ref.py) against its own invariants, hand-counted tables and the
mpmath evaluation, and the host side of `Radiomics: classes`: the names, the parser accessor, the header.  No GPU."""
import math
import os

import numpy as np
import pytest

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_texture_ref as T
from tests._radiomics_texture_cases import BOUND, EXPECT_NG, FLAGGED, MEASURED, MLP_STREAM, TEXTURE_CASES, U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TEX = {}


def _tex(name):
    if name not in _TEX:
        _TEX[name] = T.restate(TEXTURE_CASES[name])
    return _TEX[name]


@pytest.mark.parametrize("name", list(TEXTURE_CASES))
def test_tables_keep_the_histogram(name):
    tex = _tex(name)
    ref = tex["ref"]
    if name in FLAGGED:
        assert tex["flagged"] and not any(tex[k].any() for k in ("glrlm", "gldm", "ngtdm_n", "ngtdm_s"))
        assert all(math.isnan(v[0]) for f in tex["features"].values() for v in f.values())
        return
    assert not tex["flagged"]
    if name in EXPECT_NG:
        assert ref["n_bins"] == EXPECT_NG[name]
    hist, ng = ref["hist"], ref["n_bins"]
    j = np.arange(1, tex["glrlm"].shape[2] + 1)
    for d in range(13):
        assert np.array_equal((tex["glrlm"][d] * j).sum(axis=1), hist), (name, d)        # every ROI voxel is in one run per direction
    assert np.array_equal(tex["gldm"].sum(axis=1), hist) and np.array_equal(tex["ngtdm_n"].sum(axis=1), hist)
    assert tex["glrlm"][:, ng:].sum() == 0 and tex["gldm"][ng:].sum() == 0 and tex["ngtdm_s"][ng:].sum() == 0
    assert tex["ngtdm_s"][:, 0].sum() == 0                 # a voxel without neighbours has B = 0 and c = 0
    if ref["n"] <= 1200:
        assert np.array_equal(T.count_glrlm_by_walking(ref["bins"], TEXTURE_CASES[name]["max_bins"]), tex["glrlm"]), name


def test_thresholds_have_a_case_on_either_side():
    from tests._radiomics_texture_cases import FEATURE_LDS_L, NBHD_LDS_NG, RUN_LDS_WORDS
    words = {n: _tex(n)["ref"]["n_bins"] * max(TEXTURE_CASES[n]["scan"].shape) for n in ("run_ng256_l64", "run_ng300_l64", "global_ng240")}
    assert words["run_ng256_l64"] == RUN_LDS_WORDS < words["run_ng300_l64"] and words["global_ng240"] < RUN_LDS_WORDS
    assert _tex("nbhd_ng128")["ref"]["n_bins"] == NBHD_LDS_NG == _tex("nbhd_ng129")["ref"]["n_bins"] - 1
    assert max(TEXTURE_CASES["long_row"]["scan"].shape) > FEATURE_LDS_L >= 64
    assert all(b == 64 * U for b in BOUND.values())        # 8 x the measured deviation stays under the floor in every class


def test_hand_counted_constant_volume():
    tex = _tex("constant")                                  # 13 x 10 x 9, one bin, n = 1170
    P, f = tex["glrlm"], tex["features"]
    assert P[0, 0].tolist() == [0] * 12 + [90] and P[2, 0, 9] == 117 and P[8, 0, 8] == 130        # axis runs span the volume
    assert P[2, 0].sum() == 117 and P[8, 0].sum() == 130
    assert P[12, 0].sum() == 1170 - 12 * 9 * 8 and P[12, 0, 8] == 5 * 2          # (1,1,1): runs start on three faces; 9 voxels long from 5 x 2 of them
    g = tex["gldm"][0]
    assert (g[26], g[17], g[11], g[7]) == (11 * 8 * 7, 2 * (11 * 8 + 11 * 7 + 8 * 7), 4 * (11 + 8 + 7), 8) and g.sum() == 1170
    assert np.array_equal(tex["ngtdm_n"], tex["gldm"]) and tex["ngtdm_s"].sum() == 0
    x = T.matrix_features(P[0, :1], 1170)
    assert x[0][0] == pytest.approx(1.0 / 169.0, rel=1e-15) and x[1][0] == 169.0 and x[6][0] == 90.0 / 1170.0 and x[7][0] == 0.0 and x[8][0] == 0.0
    assert x[2][0] == 90.0 and x[3][0] == 1.0 and abs(x[9][0]) < 1e-15
    n = f["ngtdm"]
    assert (n["Coarseness"][0], n["Contrast"][0], n["Busyness"][0], n["Complexity"][0], n["Strength"][0]) == (1.0e6, 0.0, 0.0, 0.0, 0.0)
    assert f["gldm"]["GrayLevelVariance"][0] == 0.0 and f["gldm"]["LowGrayLevelEmphasis"][0] == 1.0
    assert f["gldm"]["LargeDependenceEmphasis"][0] == pytest.approx((616 * 27 ** 2 + 442 * 18 ** 2 + 104 * 12 ** 2 + 8 * 8 ** 2) / 1170.0, rel=1e-14)


def test_hand_counted_broken_runs():
    cut, dot = _tex("constant_plane_cleared"), _tex("constant_one_voxel")
    assert cut["glrlm"][2, 0, 3] == 117 and cut["glrlm"][2, 0, 4] == 117 and cut["glrlm"][2, 0].sum() == 234      # y runs: 4 and 5 long
    assert cut["glrlm"][0, 0].tolist() == [0] * 12 + [81]
    P = dot["glrlm"][0]                                     # the voxel (6, 4, 3) of bin 3 cuts its x run into 6 + 1 + 6
    assert dot["ref"]["n_bins"] == 3 and P[2, 0] == 1 and P[0, 5] == 2 and P[0, 12] == 89 and P.sum() == 92
    assert dot["gldm"][2].tolist() == [1] + [0] * 26 and dot["gldm"][0, 25] == 26
    assert dot["ngtdm_n"][2, 26] == 1 and dot["ngtdm_s"][2, 26] == 3 * 26 - 26 and dot["ngtdm_s"][0, 26] == 26 * 2


def test_hand_counted_checkerboard():
    tex = _tex("checkerboard")                              # bins 1 and 2 alternate: 585 voxels each
    hist = tex["ref"]["hist"]
    assert hist[:2].tolist() == [585, 585]
    for d, off in enumerate(T.DIRECTIONS):
        if sum(abs(c) for c in off) % 2 == 1:               # the neighbour along an odd offset has the other bin: every run has length 1
            assert tex["glrlm"][d, :2, 0].tolist() == [585, 585] and tex["glrlm"][d, :, 1:].sum() == 0, off
        else:
            assert tex["glrlm"][d, :2, 0].sum() < 1170, off
    inner = np.zeros((13, 10, 9), bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert tex["gldm"][:2, 12].sum() == inner.sum() == 616          # the 12 edge neighbours share the bin: dependence 13
    assert tex["gldm"][:2, 13:].sum() == 0
    assert tex["ngtdm_n"][:2, 26].sum() == 616 and tex["ngtdm_s"][:2, 26].sum() == 616 * 14       # |1 * 26 - 40| = |2 * 26 - 38| = 14
    f = T.matrix_features(tex["glrlm"][0, :2], 1170)
    assert f[0][0] == 1.0 and f[1][0] == 1.0 and f[6][0] == 1.0 and f[8][0] == 0.0 and f[7][0] == 0.25 and f[9][0] == pytest.approx(1.0)


def test_isolated_voxels_and_short_rows():
    one = _tex("single_voxel")
    assert all(math.isnan(v[0]) for v in one["features"]["ngtdm"].values())                     # Nvp = 0
    assert one["ngtdm_n"].sum() == 1 and one["ngtdm_n"][0, 0] == 1 and one["gldm"][0, 0] == 1   # counted in column 0
    assert one["features"]["glrlm"]["RunPercentage"][0] == 1.0 and one["features"]["gldm"]["SmallDependenceEmphasis"][0] == 1.0
    for n in (2, 3, 4):
        tex = _tex(f"n{n}")
        assert tex["ngtdm_n"][:, 0].sum() == 0 and tex["ngtdm_n"][:, 1].sum() == 2 and tex["ngtdm_n"][:, 2].sum() == n - 2
        assert all(math.isfinite(v[0]) for v in tex["features"]["ngtdm"].values())


@pytest.mark.parametrize("name", [n for n in TEXTURE_CASES if n not in FLAGGED])
def test_restatement_stays_within_its_own_bound(name):
    tex = _tex(name)
    values = {cls: {k: v[0] for k, v in f.items()} for cls, f in tex["features"].items()}
    dev = T.deviations(tex, values, T.exact(tex))
    for cls, d in dev.items():
        assert d <= MEASURED[cls], (name, cls, d / U)


# ---- names, parser, header ---------------------------------------------------------------------------------------------------------------
def test_feature_names():
    assert radiomics.feature_names() == radiomics.FEATURE_NAMES and radiomics.feature_names(()) == radiomics.FEATURE_NAMES
    assert len(radiomics.FEATURE_NAMES) == 47
    every = radiomics.feature_names(radiomics.TEXTURE_CLASSES)
    assert len(every) == 82 and len(set(every)) == 82 and every[:47] == radiomics.FEATURE_NAMES
    assert every[47] == "original_glrlm_ShortRunEmphasis" and every[63] == "original_gldm_SmallDependenceEmphasis" and every[-1] == "original_ngtdm_Strength"
    assert [len(radiomics.feature_names([c])) for c in radiomics.TEXTURE_CLASSES] == [63, 61, 52]
    assert radiomics.feature_names(["ngtdm", "glrlm"]) == radiomics.feature_names(["glrlm", "ngtdm"])      # the order is fixed
    assert radiomics.feature_names("all") == every and radiomics.texture_classes("gldm,glrlm") == ("glrlm", "gldm")
    assert (radiomics.GLRLM, radiomics.GLDM, radiomics.NGTDM) == (T.GLRLM, T.GLDM, T.NGTDM)
    assert radiomics.TEXTURE_CLASSES == ("glrlm", "gldm", "ngtdm")
    assert (_lib.RADIOMICS_GLRLM, _lib.RADIOMICS_GLDM, _lib.RADIOMICS_NGTDM) == (16, 14, 5) and _lib.RADIOMICS_TEXTURE_BYTES == 35 * 8
    with pytest.raises(ConfigurationError, match="glrlm, gldm, ngtdm"):
        radiomics.feature_names(["glszm"])


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
    assert _parser(tmp_path, None).radiomicsClasses() == ()
    assert _parser(tmp_path, {"bin_width": 10}).radiomicsClasses() == ()
    p = _parser(tmp_path, {"bin_width": 10, "max_bins": 128, "classes": ["ngtdm", "glrlm"]})
    assert p.radiomicsClasses() == ("glrlm", "ngtdm")
    assert p.radiomicsConfig() == {"bin_width": 10.0, "max_bins": 128, "standardize": True}
    assert _parser(tmp_path, {"classes": ["glrlm", "gldm", "ngtdm"]}).radiomicsClasses() == radiomics.TEXTURE_CLASSES
    with pytest.raises(ConfigurationError, match="glszm.*glrlm, gldm, ngtdm"):
        _parser(tmp_path, {"classes": ["glrlm", "glszm"]}).radiomicsClasses()
    with pytest.raises(ConfigurationError, match="classes"):
        _parser(tmp_path, {"classes": 3}).radiomicsClasses()


def test_header_declares_the_texture_call():
    header = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    for word in ("int64_t mmnn_radiomics_texture_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins);",
                 "int mmnn_radiomics_texture(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws,",
                 "#define MMNN_RADIOMICS_GLRLM 16", "#define MMNN_RADIOMICS_GLDM 14", "#define MMNN_RADIOMICS_NGTDM 5",
                 "} mmnn_radiomics_texture_result;"):
        assert word in header, word
    for name in T.GLRLM + T.GLDM + T.NGTDM:
        assert name in header, name


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
