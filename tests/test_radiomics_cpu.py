"""The numpy restatement of the radiomic features (tests/_radiomics_ref.py) against independent closed forms, and the host side of
`--radiomics`: the csv, the datasets, the scaler, the parser / model wiring and the refusals.  No GPU."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mmnn_sts_amd import radiomics
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests import _radiomics_ref as R
from tests._radiomics_cases import BOUND, CASES, MEASURED, U


def _restate(name):
    c = CASES[name]
    with np.errstate(all="ignore"):
        return R.restate(c["scan"], c["mask"], c["bin_width"], c["max_bins"], c["scan_scale"], c["mask_scale"])


def test_feature_names():
    assert len(radiomics.FEATURE_NAMES) == 47 and len(set(radiomics.FEATURE_NAMES)) == 47
    assert radiomics.FEATURE_NAMES[0] == "original_firstorder_Energy" and "original_shape_VoxelVolume" in radiomics.FEATURE_NAMES
    assert radiomics.FEATURE_NAMES[-1] == "original_glcm_SumSquares" and "original_firstorder_10Percentile" in radiomics.FEATURE_NAMES
    assert radiomics.DEVICE_FIRSTORDER == R.FIRSTORDER and radiomics.GLCM == R.GLCM
    assert all(b == 64 * U for b in BOUND.values())      # 8 x the measured deviation stays under the floor in every class


@pytest.mark.parametrize("name", ["ellipsoid", "seven_levels", "scan_float64", "global_ng240"])
def test_first_order_against_scipy_and_numpy(name):
    from scipy import stats
    ref = _restate(name)
    v, fo = ref["values"], ref["firstorder"]
    assert fo["Skewness"][0] == pytest.approx(stats.skew(v), rel=1e-12, abs=1e-13)
    assert fo["Kurtosis"][0] == pytest.approx(stats.kurtosis(v, fisher=False), rel=1e-12)
    for k, p in (("10Percentile", 10), ("90Percentile", 90), ("Median", 50)):
        assert fo[k][0] == pytest.approx(np.percentile(v, p), rel=1e-12, abs=1e-300)
    assert fo["InterquartileRange"][0] == pytest.approx(np.percentile(v, 75) - np.percentile(v, 25), rel=1e-12)
    assert fo["Variance"][0] == pytest.approx(np.var(v), rel=1e-12) and fo["Energy"][0] == pytest.approx(float(np.dot(v, v)), rel=1e-12)
    assert fo["Range"][0] == v.max() - v.min() and fo["Mean"][0] == pytest.approx(v.mean(), rel=1e-13)
    s = np.sort(v)
    n = len(v)
    assert np.array_equal(ref["order"], [s[int(f((n - 1) * p / 100.0))] for p in R.PCT for f in (math.floor, math.ceil)])
    assert ref["hist"].sum() == n and ref["hist"][ref["n_bins"]:].sum() == 0 and ref["hist"][ref["n_bins"] - 1] > 0


def test_hand_counted_glcm_of_a_row():
    row = np.array([1, 2, 1, 2], dtype=np.int16).reshape(4, 1, 1)
    ref = R.restate(row, np.ones_like(row, dtype=np.uint8), 1.0, 4)
    assert ref["n_bins"] == 2 and ref["hist"].tolist() == [2, 2, 0, 0]
    assert ref["glcm"][0][:2, :2].tolist() == [[0, 3], [3, 0]] and ref["glcm"][1:].sum() == 0 and ref["glcm"].sum() == 6
    f = ref["glcm_features"]
    assert f["Contrast"][0] == 1.0 and f["JointAverage"][0] == 1.5 and f["MaximumProbability"][0] == 0.5
    assert f["Correlation"][0] == pytest.approx(-1.0) and f["JointEntropy"][0] == pytest.approx(1.0) and f["Autocorrelation"][0] == 2.0


def test_hand_counted_glcm_of_a_cube():
    cube = np.zeros((2, 2, 2), dtype=np.int16)
    cube[1] = 1                                           # value = x: bins 1 and 2
    ref = R.restate(cube + 1, np.ones((2, 2, 2), np.uint8), 1.0, 2)
    off, same = lambda k: [[0, k], [k, 0]], lambda k: [[k, 0], [0, k]]
    want = {(0, 0, 1): off(4), (0, 1, -1): off(2), (0, 1, 0): same(4), (0, 1, 1): off(2), (1, -1, -1): off(1), (1, -1, 0): same(2),
            (1, -1, 1): off(1), (1, 0, -1): off(2), (1, 0, 0): same(4), (1, 0, 1): off(2), (1, 1, -1): off(1), (1, 1, 0): same(2), (1, 1, 1): off(1)}
    assert list(want) == R.DIRECTIONS
    for d, key in enumerate(R.DIRECTIONS):
        assert ref["glcm"][d].tolist() == want[key], key


def test_box_roi_axis_lengths():
    mask = np.zeros((20, 18, 12), dtype=np.uint8)
    mask[3:14, 2:9, 4:9] = 1                              # 11 x 7 x 5 voxels
    ref = R.restate(np.ones(mask.shape, np.int16), mask)
    spacing = (0.9, 1.5, 3.0)
    got = radiomics.shape_features(ref["n"], ref["moments"], np.diag(spacing))
    lengths = sorted((4.0 * math.sqrt((m * m - 1) / 12.0) * s for m, s in zip((11, 7, 5), spacing)), reverse=True)
    for k, v in zip(("MajorAxisLength", "MinorAxisLength", "LeastAxisLength"), lengths):
        assert got[k] == pytest.approx(v, rel=1e-12)
    assert got["VoxelVolume"] == pytest.approx(11 * 7 * 5 * 0.9 * 1.5 * 3.0, rel=1e-14)
    assert got["Elongation"] == pytest.approx(lengths[1] / lengths[0], rel=1e-12) and got["Flatness"] == pytest.approx(lengths[2] / lengths[0], rel=1e-12)
    assert ref["lo"].tolist() == [3, 2, 4] and ref["hi"].tolist() == [13, 8, 8]
    rot = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]) @ np.diag(spacing)
    got, want = radiomics.shape_features(ref["n"], ref["moments"], rot), R.shape_reference(mask != 0, rot)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-11)


def test_flat_roi():
    mask = np.zeros((6, 5, 4), dtype=np.uint8)
    mask[1:5, 1:4, 1:3] = 1
    ref = R.restate(np.full(mask.shape, 37, np.int16), mask)
    fo, g = ref["firstorder"], ref["glcm_features"]
    assert ref["n_bins"] == 1 and fo["Skewness"][0] == 0.0 and fo["Kurtosis"][0] == 0.0 and fo["Variance"][0] == 0.0
    assert g["Correlation"][0] == 1.0 and g["Imc1"][0] == 0.0 and g["Imc2"][0] == 0.0 and g["JointEnergy"][0] == 1.0
    assert fo["Uniformity"][0] == 1.0 and abs(fo["Entropy"][0]) < 1e-15


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_stays_within_its_own_bound(name):
    ref = _restate(name)
    if ref["empty"] or ref["nonfinite"] or ref["overflow"]:
        assert all(math.isnan(v[0]) for v in ref["firstorder"].values()) and all(math.isnan(v[0]) for v in ref["glcm_features"].values())
        assert ref["hist"].sum() == 0 and ref["glcm"].sum() == 0
        return
    values = {k: R.value_and_scale(ref, k)[0] for names in R.CLASSES.values() for k in names}
    dev = R.deviations(ref, values)
    for cls, d in dev.items():
        assert d <= MEASURED[cls], (name, cls, d / U)


# ---- the csv and the datasets --------------------------------------------------------------------------------------------------------------
def _clinical(path, uids):
    from mmnn_sts_amd.data.constants import NUM_CLASSES
    cols = ["uid"] + [f"predictor{i}" for i in range(32)] + [f"event{i}" for i in range(NUM_CLASSES)] + [f"duration{i}" for i in range(NUM_CLASSES)]
    rng = np.random.default_rng(3)
    rows = np.concatenate([np.asarray(uids, dtype=np.float64)[:, None], rng.standard_normal((len(uids), 32)),
                           (rng.random((len(uids), NUM_CLASSES)) < 0.6).astype(np.float64), rng.integers(1, 900, (len(uids), NUM_CLASSES)).astype(np.float64)], axis=1)
    np.savetxt(path, rows, delimiter=",", header=",".join(cols), comments="", fmt="%.9g")
    return str(path)


def _rows(uids, prefixes=("",), seed=0):
    rng = np.random.default_rng(seed)
    return [dict({"MRN": u}, **{p + n: float(rng.standard_normal() * 10.0 ** rng.integers(-3, 6)) for p in prefixes for n in radiomics.FEATURE_NAMES}) for u in uids]


def test_csv_round_trip(tmp_path):
    rows = _rows([1000, 1007, 1014], ("t1_", "t2_"))
    rows[0]["t1_original_firstorder_Energy"] = 0.1 + 0.2
    radiomics.write_csv(tmp_path / "r.csv", rows)
    cols, back = radiomics.read_csv(tmp_path / "r.csv")
    assert cols == ["MRN"] + [p + n for p in ("t1_", "t2_") for n in radiomics.FEATURE_NAMES] and len(cols) == 95
    for r, b in zip(rows, back):
        assert int(b[0]) == r["MRN"] and [float(x) for x in b[1:]] == [r[c] for c in cols[1:]]      # repr round-trips every bit


def test_survival_dataset_over_a_csv_and_a_pyradiomics_csv(tmp_path):
    from mmnn_sts_amd.data.RadiomicsDatasets import RadiomicsClassificationDataset, RadiomicsSurvivalDataset
    uids = [1000, 1007, 1014, 1021]
    clin = _clinical(tmp_path / "clinical.csv", uids + [1028])
    rows = _rows(uids)
    radiomics.write_csv(tmp_path / "r.csv", rows)
    ds = RadiomicsSurvivalDataset(str(tmp_path / "r.csv"), clin)
    assert ds.uids == uids and len(ds) == 4 and ds.columns == list(radiomics.FEATURE_NAMES) and ds.multimodal_identifier == "clinical"
    x, ev, du = ds.getDataByUID(1014)
    assert x.dtype == torch.float32 and x.shape == (47,) and torch.equal(ev, ds.labels.events(1014)) and torch.equal(du, ds.labels.durations(1014))
    assert torch.equal(x, torch.tensor([rows[2][n] for n in radiomics.FEATURE_NAMES], dtype=torch.float64).float())
    assert len(RadiomicsClassificationDataset(str(tmp_path / "r.csv"), clin)[0]) == 2
    # a PyRadiomics csv: provenance columns, a label column, an excluded one
    cols, body = radiomics.read_csv(tmp_path / "r.csv")
    with open(tmp_path / "p.csv", "w") as f:
        f.write(",".join(["diagnostics_Versions_PyRadiomics", "diagnostics_Image-original_Hash", "MRN", "label", "original_shape_Maximum3DDiameter"] + cols[1:]) + "\n")
        for b in body:
            f.write(",".join(["v3.0.1", "abc123", b[0], "1", "55.5"] + b[1:]) + "\n")
    assert RadiomicsSurvivalDataset(str(tmp_path / "p.csv"), clin, ["original_shape_Maximum3DDiameter"]).columns == ["label"] + ds.columns
    ds2 = RadiomicsSurvivalDataset(str(tmp_path / "p.csv"), clin, ["original_shape_Maximum3DDiameter"], ["label"])
    assert ds2.columns == ds.columns and torch.equal(ds2.getDataByUID(1007)[0], ds.getDataByUID(1007)[0])
    # a cell that is no finite number names the patient and the column
    bad = [list(b) for b in body]
    bad[1][cols.index("original_glcm_Imc2")] = "nan"
    with open(tmp_path / "bad.csv", "w") as f:
        f.write(",".join(cols) + "\n" + "".join(",".join(b) + "\n" for b in bad))
    with pytest.raises(ConfigurationError, match=r"patient 1007, column original_glcm_Imc2"):
        RadiomicsSurvivalDataset(str(tmp_path / "bad.csv"), clin)
    bad[1][cols.index("original_glcm_Imc2")] = "see note"
    with open(tmp_path / "bad.csv", "w") as f:
        f.write(",".join(cols) + "\n" + "".join(",".join(b) + "\n" for b in bad))
    with pytest.raises(ConfigurationError, match=r"patient 1007, column original_glcm_Imc2"):
        RadiomicsSurvivalDataset(str(tmp_path / "bad.csv"), clin)
    with pytest.raises(ConfigurationError, match="no row in the clinical csv"):
        RadiomicsSurvivalDataset(str(tmp_path / "r.csv"), _clinical(tmp_path / "short.csv", uids[:3]))


def test_scaler_is_fitted_on_the_training_uids_and_reloaded(tmp_path):
    from mmnn_sts_amd.data.RadiomicsDatasets import RadiomicsSurvivalDataset
    uids = [1000, 1007, 1014, 1021, 1028]
    clin = _clinical(tmp_path / "clinical.csv", uids)
    rows = _rows(uids, seed=4)
    for r in rows:
        r["original_glcm_Id"] = 2.5                         # a constant column: std 0 -> 1
    radiomics.write_csv(tmp_path / "r.csv", rows)
    ds = RadiomicsSurvivalDataset(str(tmp_path / "r.csv"), clin)
    train = [1000, 1014, 1028]
    table = np.array([[r[n] for n in radiomics.FEATURE_NAMES] for r in rows])
    mean, std = ds.fit_scaler(train)
    assert np.array_equal(mean, table[[0, 2, 4]].mean(axis=0))
    want_std = table[[0, 2, 4]].std(axis=0)
    want_std[list(radiomics.FEATURE_NAMES).index("original_glcm_Id")] = 1.0
    assert np.array_equal(std, want_std)
    z = torch.stack([ds.getDataByUID(u)[0] for u in train]).double().numpy()
    assert np.allclose(z.mean(axis=0), 0.0, atol=1e-6) and np.allclose(np.delete(z.std(axis=0), list(radiomics.FEATURE_NAMES).index("original_glcm_Id")), 1.0, atol=1e-5)
    ds.save_scaler(tmp_path / "radiomics_scaler.csv")
    again = RadiomicsSurvivalDataset(str(tmp_path / "r.csv"), clin)
    assert not torch.equal(again.getDataByUID(1007)[0], ds.getDataByUID(1007)[0])
    again.load_scaler(tmp_path / "radiomics_scaler.csv")
    assert np.array_equal(again.mean, ds.mean) and np.array_equal(again.std, ds.std)
    assert torch.equal(again.getDataByUID(1007)[0], ds.getDataByUID(1007)[0])
    other = RadiomicsSurvivalDataset(str(tmp_path / "r.csv"), clin, exclude_columns=["original_glcm_Idn"])
    with pytest.raises(ConfigurationError, match="other columns"):
        other.load_scaler(tmp_path / "radiomics_scaler.csv")


# ---- parser, models, main ---------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    base = dict(images=False, preop=False, postop=False, radiomics=True, survival=True, classification=False, blend=False, rad_loc=None,
                image_loc=None, data_loc=None, key_loc=None)
    base.update(kw)
    return SimpleNamespace(**base)


def _parser(tmp_path, rad, clin, **radiomics_model):
    import yaml
    from mmnn_sts_amd.parser.parser import Parser
    cfg = {"ImageModel": {"name": "tinydensenet", "modality": "t1t2", "feature_layers": 12, "num_classes": 2, "spatial_dims": 3, "in_channels": 2,
                          "dropout_prob": 0.2},
           "ClinicalModel": {"NUM_PREDICTORS": 32, "PRE_OP_PREDICTORS": [], "POST_OP_PREDICTORS": []},
           "Hyperparameters": {"train_batch_size": 2}, "Data": {"rad_loc": rad, "data_loc": clin}, "Radiomics": {"bin_width": 10, "max_bins": 128}}
    if radiomics_model:
        cfg["RadiomicsModel"] = radiomics_model
    (tmp_path / "c.yaml").write_text(yaml.safe_dump(cfg))
    p = Parser(str(tmp_path / "c.yaml"))
    p.parseConfig()
    return p


@pytest.mark.parametrize("prefixes,preop,width", [(("",), False, 47), (("t1_", "t2_"), False, 94), (("t1_", "t2_"), True, 126)])
def test_parser_and_model_widths(tmp_path, prefixes, preop, width):
    from mmnn_sts_amd.data.RadiomicsDatasets import JoinedTableDataset, RadiomicsSurvivalDataset
    from mmnn_sts_amd.models.mlp import MLP
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    uids = [1000, 1007, 1014, 1021]
    clin = _clinical(tmp_path / "clinical.csv", uids)
    radiomics.write_csv(tmp_path / "r.csv", _rows(uids, prefixes))
    p = _parser(tmp_path, str(tmp_path / "r.csv"), clin)
    assert p.radiomicsConfig() == {"bin_width": 10.0, "max_bins": 128, "standardize": True}
    a = _args(preop=preop)
    p.applyDataFlags(a)
    assert len(p.predictors(a)) == width and p.predictors(a)[-1] == prefixes[-1] + "original_glcm_SumSquares"
    ds = p.getDatasets(a)
    assert isinstance(ds, JoinedTableDataset if preop else RadiomicsSurvivalDataset) and ds.uids == uids
    x, ev, du = ds.getDataByUID(1007)
    assert x.shape == (width,) and ev.shape == du.shape
    if preop:
        assert ds.predictors[:32] == [f"predictor{i}" for i in range(32)] and torch.equal(x[:32], ds.tables[0].getDataByUID(1007)[0])
        assert torch.equal(x[32:], ds.tables[1].getDataByUID(1007)[0])
    m = p.getModel(a)
    assert isinstance(m, MLP) and m.in_channels == width and m.backbone.dense0.weight.shape == (32, width)
    fused = p.getModel(_args(preop=preop, images=True))
    assert isinstance(fused, MultiModalModel) and fused.num_clinical_inputs == width and fused.clinical_model.model.backbone.dense0.weight.shape == (32, width)


def test_main_refusals(tmp_path, monkeypatch):
    import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match=r"--rad_loc.*--image_loc"):
        main.main(["--radiomics", "--survival"])
    with pytest.raises(SystemExit, match=r"--segmentation is outside"):
        main.main(["--segmentation", "--radiomics"])
    with pytest.raises(SystemExit, match=r"--data_loc"):
        main.main(["--radiomics", "--survival", "--rad_loc", str(tmp_path / "r.csv")])
    with pytest.raises(SystemExit, match=r"--data_loc and --key_loc"):
        main.main(["--radiomics", "--survival", "--image_loc", str(tmp_path)])
    with pytest.raises(SystemExit, match=r"needs --image_loc"):
        main.main(["--radiomics", "--images", "--survival", "--rad_loc", str(tmp_path / "r.csv"), "--data_loc", str(tmp_path / "c.csv")])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match=r"single process.*--rad_loc"):
        main.main(["--radiomics", "--survival", "--image_loc", str(tmp_path), "--data_loc", "c.csv", "--key_loc", "k.csv"])


def test_stacked_layout_of_every_switch_combination():
    """The one read-back's layout, from the module docstring and the `_lib.RADIOMICS_*` sizes: per image (the original, then each LoG
    scale ascending) the result block, then the texture block if any class was asked for, the size-zone block, the mesh block (original
    only).  Word k of the buffer holds the double k, so a device-computed column must hold the index of the word it is read from."""
    from itertools import combinations, product
    from mmnn_sts_amd import _lib
    L = _lib
    first = L.RADIOMICS_RESULT_INT64 + len(radiomics.ORDER_RANKS)
    assert (first + L.RADIOMICS_FIRSTORDER + L.RADIOMICS_GLCM) * 8 == L.RADIOMICS_RESULT_BYTES
    tex_off = {"glrlm": 0, "gldm": L.RADIOMICS_GLRLM, "ngtdm": L.RADIOMICS_GLRLM + L.RADIOMICS_GLDM}
    tex_names = {"glrlm": radiomics.GLRLM, "gldm": radiomics.GLDM, "ngtdm": radiomics.NGTDM}
    subsets = [c for k in range(4) for c in combinations(radiomics.TEXTURE_CLASSES, k)]
    combos = list(product(subsets, (False, True), (False, True), ((), (1.0,), (1.0, 3.0))))
    assert len(combos) == 96
    for classes, glszm, mesh, sigmas in combos:
        expect, words, starts = {}, 0, []
        for image in ("original",) + tuple(radiomics.log_image_type(s) for s in sigmas):
            starts.append(words)
            for j, n in enumerate(radiomics.DEVICE_FIRSTORDER):
                expect[f"{image}_firstorder_{n}"] = words + first + j
            for j, n in enumerate(radiomics.GLCM):
                expect[f"{image}_glcm_{n}"] = words + first + L.RADIOMICS_FIRSTORDER + j
            words += L.RADIOMICS_RESULT_BYTES // 8
            if classes:
                for c in classes:
                    for j, n in enumerate(tex_names[c]):
                        expect[f"{image}_{c}_{n}"] = words + tex_off[c] + j
                words += L.RADIOMICS_TEXTURE_BYTES // 8
            if glszm:
                for j, n in enumerate(radiomics.GLSZM):
                    expect[f"{image}_glszm_{n}"] = words + (L.RADIOMICS_ZONES_BYTES // 8 - L.RADIOMICS_GLSZM) + j
                words += L.RADIOMICS_ZONES_BYTES // 8
            if mesh and image == "original":
                words += L.RADIOMICS_MESH_BYTES // 8
        buf = np.arange(words, dtype=np.float64)
        for s in starts:                  # n = 8; lo, hi; the index sums of the block (0..1)^3; n_bins; the three flags clear
            buf[s:s + L.RADIOMICS_RESULT_INT64].view(np.int64)[:] = [8, 0, 0, 0, 1, 1, 1, 4, 4, 4, 4, 4, 4, 2, 2, 2, 2, 0, 0, 0]

        def result(image, with_mesh):
            return radiomics.RadiomicsResult(None, None, None, None, (2, 2, 2), None, 25.0, 256, classes=classes, glszm=glszm,
                                             mesh_shape=with_mesh, linear=np.eye(3) if with_mesh else None, image=image)
        r = result("original", mesh)
        r.log = tuple((s, result(radiomics.log_image_type(s), False)) for s in sigmas)
        got = radiomics._features_of_stacked(buf.view(np.uint8), r, None, "layout")
        assert tuple(got) == radiomics.feature_names(classes, glszm, mesh, sigmas), (classes, glszm, mesh, sigmas)
        assert {k: got[k] for k in expect} == {k: float(v) for k, v in expect.items()}, (classes, glszm, mesh, sigmas)
        assert len(got) - len(expect) == (1 + len(sigmas)) + len(radiomics.SHAPE) + (len(radiomics.MESH_SHAPE) if mesh else 0)
