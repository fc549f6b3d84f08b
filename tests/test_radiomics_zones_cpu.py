"""The numpy / scipy restatement of the size-zone class (tests/_radiomics_zones_ref.py) against an independent flood fill, hand-counted
zones, its own invariants and the mpmath evaluation, and the host side of `Radiomics: glszm`: the names, the parser accessor, the header,
the constants of the binding.  No GPU."""
import math
import os

import numpy as np
import pytest

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_zones_ref as Z
from tests._radiomics_zones_cases import BOUND, EXPECT, FLAGGED, FROM_TEXTURE, MEASURED, MLP_STREAM, ROW_WRAP, SMALL, U, ZONE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ZN = {}


def _zn(name):
    if name not in _ZN:
        _ZN[name] = Z.restate(ZONE_CASES[name])
    return _ZN[name]


def test_the_cases_the_issue_names_are_all_here():
    from tests._radiomics_texture_cases import TEXTURE_CASES
    assert len(FROM_TEXTURE) == 24 and all(ZONE_CASES[k] is TEXTURE_CASES[k] for k in FROM_TEXTURE)
    assert set(ZONE_CASES) - set(FROM_TEXTURE) == {"corner_stairs", "row_wrap", "serpentine", "comb", "lattice", "noise_ng8", "noise_ng2", "big_zone"}
    assert {"corner_stairs", "row_wrap", "comb", "six_faces", "constant", "checkerboard"} <= set(SMALL)
    assert all(b == 64 * U for b in BOUND.values())        # 8 x the measured deviation stays under the floor in both classes


@pytest.mark.parametrize("name", [n for n in SMALL if n not in FLAGGED])
def test_scipy_labelling_equals_the_flood_fill(name):
    zn = _zn(name)
    labels, sizes = Z.flood_fill(zn["bins"])
    assert np.array_equal(Z.flat(labels), zn["labels"]) and np.array_equal(Z.flat(sizes), zn["sizes"])


@pytest.mark.parametrize("name", list(ZONE_CASES))
def test_invariants(name):
    zn = _zn(name)
    if name in FLAGGED:
        assert zn["flagged"] and not zn["labels"].any() and not zn["sizes"].any() and not zn["levels"].any()
        assert not any(zn["integers"].values()) and all(math.isnan(v[0]) for v in zn["features"].values())
        return
    assert not zn["flagged"]
    n, ng, I = zn["ref"]["n"], zn["ref"]["n_bins"], zn["integers"]
    bins = Z.flat(zn["bins"])
    assert zn["sizes"].sum() == n and I["nz"] == zn["levels"].sum() == np.count_nonzero(zn["sizes"]) and zn["levels"][ng:].sum() == 0
    assert I["n_keys"] <= math.sqrt(2 * n * ng) and I["max_size"] == zn["sizes"].max()
    assert np.array_equal(zn["labels"] > 0, bins > 0)
    roots = np.flatnonzero(zn["sizes"])
    assert np.array_equal(zn["labels"][roots], roots + 1)                                  # a root carries its own index
    assert np.array_equal(np.bincount(zn["labels"][bins > 0] - 1, minlength=len(bins))[roots], zn["sizes"][roots])
    assert (zn["labels"][bins > 0] - 1 <= np.flatnonzero(bins > 0)).all()                 # the label is the zone's smallest index
    assert np.array_equal(bins[zn["labels"][bins > 0] - 1], bins[bins > 0])               # one bin per zone
    assert all(math.isfinite(v[0]) for v in zn["features"].values())                       # no feature degenerates while n > 0
    if name in EXPECT:
        want = EXPECT[name]
        assert (I["nz"], I["max_size"], I["n_keys"]) == want, (name, I)


def test_hand_counted_zones():
    assert sorted(_zn("constant")["sizes"][_zn("constant")["sizes"] > 0]) == [1170]
    assert sorted(_zn("constant_plane_cleared")["sizes"][_zn("constant_plane_cleared")["sizes"] > 0]) == [468, 585]
    assert sorted(_zn("checkerboard")["sizes"][_zn("checkerboard")["sizes"] > 0]) == [585, 585]        # diagonals connect
    assert _zn("run_ng300_l64")["integers"]["nz"] == 8874 and _zn("run_ng300_l64")["integers"]["n_keys"] == 503
    stairs = _zn("corner_stairs")
    assert stairs["sizes"][0] == 8 and stairs["integers"]["nz"] == 1 and set(stairs["labels"]) == {0, 1}
    wrap = _zn("row_wrap")
    lin = sorted(x + 5 * (y + 4 * z) for x, y, z in ROW_WRAP)
    assert np.flatnonzero(wrap["sizes"]).tolist() == lin and wrap["sizes"][lin].tolist() == [1, 1, 1, 1] and lin[1] == lin[0] + 1 and lin[3] == lin[2] + 1
    assert wrap["labels"][lin].tolist() == [v + 1 for v in lin]
    snake = _zn("serpentine")
    on = np.flatnonzero(snake["labels"])
    assert snake["sizes"][0] == 899 and (snake["labels"][on] == 1).all() and on[-1] == 24 * 23 * 5 - 1       # from the first voxel to the last
    assert sorted(_zn("comb")["sizes"][_zn("comb")["sizes"] > 0]) == [89, 89]
    lat = _zn("lattice")
    assert lat["integers"]["nz"] == 256 and lat["levels"][:3].sum() == 256 and (lat["levels"][:3] > 0).all() and lat["integers"]["sum_ps2"] == 256 ** 2
    assert _zn("big_zone")["integers"]["max_size"] == 73728 > 65535 and _zn("big_zone")["integers"]["sum_j2"] == 73728 ** 2
    f = _zn("constant")["features"]
    assert f["SmallAreaEmphasis"][0] == pytest.approx(1.0 / 1170 ** 2, rel=1e-15) and f["LargeAreaEmphasis"][0] == 1170.0 ** 2
    assert f["ZonePercentage"][0] == 1.0 / 1170 and f["GrayLevelVariance"][0] == 0.0 and f["ZoneVariance"][0] == 0.0 and abs(f["ZoneEntropy"][0]) < 1e-15
    f = _zn("lattice")["features"]
    assert f["SmallAreaEmphasis"][0] == 1.0 and f["ZonePercentage"][0] == 1.0 and f["ZoneVariance"][0] == 0.0 and f["SizeZoneNonUniformityNormalized"][0] == 1.0


@pytest.mark.parametrize("name", [n for n in ZONE_CASES if n not in FLAGGED])
def test_restatement_stays_within_its_own_bound(name):
    zn = _zn(name)
    dev = Z.deviations(zn, {k: v[0] for k, v in zn["features"].items()}, Z.exact(zn))
    for cls, d in dev.items():
        assert d <= MEASURED[cls], (name, cls, d / U)


# ---- names, parser, header, binding --------------------------------------------------------------------------------------------------------
def test_feature_names():
    assert radiomics.GLSZM == Z.GLSZM and len(radiomics.GLSZM) == 16
    for classes in ((), ["glrlm"], ["ngtdm", "gldm"], radiomics.TEXTURE_CLASSES, "all"):
        plain, wide = radiomics.feature_names(classes), radiomics.feature_names(classes, glszm=True)
        assert radiomics.feature_names(classes, glszm=False) == plain and wide[:len(plain)] == plain
        assert wide[len(plain):] == tuple(f"original_glszm_{n}" for n in Z.GLSZM)
    assert radiomics.feature_names() == radiomics.FEATURE_NAMES and len(radiomics.feature_names("all")) == 82
    assert len(radiomics.feature_names(glszm=True)) == 63 and len(radiomics.feature_names("all", True)) == 98
    assert len(set(radiomics.feature_names("all", True))) == 98
    assert radiomics.feature_names("all", True)[82] == "original_glszm_SmallAreaEmphasis"
    assert radiomics.feature_names("all", True)[-1] == "original_glszm_LargeAreaHighGrayLevelEmphasis"
    assert radiomics.TEXTURE_CLASSES == ("glrlm", "gldm", "ngtdm")
    with pytest.raises(ConfigurationError, match="glszm.*glrlm, gldm, ngtdm.*Radiomics: glszm"):
        radiomics.feature_names(["glszm"])
    with pytest.raises(ConfigurationError) as e:
        radiomics.feature_names(["glcm2"])
    assert "Radiomics: glszm" not in str(e.value)


def test_binding_constants_and_unpack():
    assert _lib.RADIOMICS_GLSZM == 16 and _lib.RADIOMICS_ZONES_BYTES == (6 + 16) * 8 == 176
    raw = np.concatenate([np.arange(1, 7, dtype=np.int64).view(np.uint8), np.arange(16, dtype=np.float64).view(np.uint8)])
    got = radiomics.unpack_zones(raw)
    assert [got[k] for k in Z.INTEGERS] == [1, 2, 3, 4, 5, 6] and got["glszm"].tolist() == list(range(16))
    fields = {f.name for f in radiomics.RadiomicsResult.__dataclass_fields__.values()}
    assert {"zones", "labels", "sizes", "levels", "zones_workspace", "glszm"} <= fields


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
    assert _parser(tmp_path, None).radiomicsZones() is False
    assert _parser(tmp_path, {"bin_width": 10}).radiomicsZones() is False
    assert _parser(tmp_path, {"glszm": False}).radiomicsZones() is False
    p = _parser(tmp_path, {"bin_width": 10, "max_bins": 128, "classes": ["ngtdm"], "glszm": True})
    assert p.radiomicsZones() is True and p.radiomicsClasses() == ("ngtdm",)
    assert p.radiomicsConfig() == {"bin_width": 10.0, "max_bins": 128, "standardize": True}          # exactly its three keys
    for bad in ("yes", 1, ["glszm"], None):
        with pytest.raises(ConfigurationError, match="glszm"):
            _parser(tmp_path, {"glszm": bad}).radiomicsZones()


def test_header_declares_the_zones_call():
    header = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    for word in ("int64_t mmnn_radiomics_zones_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins);",
                 "int mmnn_radiomics_zones(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws,",
                 "mmnn_radiomics_zones_result* out, uint32_t* labels, uint32_t* sizes, uint32_t* levels,",
                 "#define MMNN_RADIOMICS_GLSZM 16", "} mmnn_radiomics_zones_result;"):
        assert word in header, word
    for name in Z.GLSZM + Z.INTEGERS:
        assert name in header, name


@pytest.mark.parametrize("width", sorted(MLP_STREAM))
def test_mlp_input_stream_is_the_first_well_conditioned_one(width):
    """The rule beside MLP_STREAM of tests/_radiomics_texture_cases.py: off the ReLU branch points, and torch's own fp32 evaluation within
    a quarter of the bar of the fp64 one."""
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
