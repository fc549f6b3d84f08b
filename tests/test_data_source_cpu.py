"""`main.build_data_source` for the selections that need no device: a clinical csv (synthetic, or `--data_loc`) and a radiomics table."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import main as M  # noqa: E402
from tests._cli import tiny_config  # noqa: E402


def _source(argv, rank=0, world=1):
    a = M.build_arg_parser().parse_args(argv)
    parser = M.Parser(a.config)
    M.resolve_settings(a, parser)
    return M.build_data_source(a, parser, rank, world), a, parser


# --synthetic_patients -> the rows of the train and validation csv (max(4, n), max(4, n // 4)); inference evaluates the validation csv
@pytest.mark.parametrize("task", ["--classification", "--survival"])
@pytest.mark.parametrize("n,n_train,n_val", [(4, 4, 4), (16, 16, 4), (17, 17, 4)])
def test_tabular_sets_from_the_synthetic_csv(tmp_path, n, n_train, n_val, task):
    data, a, parser = _source(["--preop", task, "--synthetic_patients", str(n), "--output_path", str(tmp_path / "out"), "--config", tiny_config(tmp_path)])
    assert (len(data.train), len(data.val), len(data.evaluation)) == (n_train, n_val, n_val)
    assert data.collate is M.collate and data.ingest is None and data.cache is None and (data.train_tf, data.val_tf) == (None, None)
    predictors = parser.predictors(a)
    assert len(predictors) == 32 and data.train[0][0].shape == (32,)
    for name, rows, seed in (("synthetic_train_rank0.csv", n_train, 1000), ("synthetic_val_rank0.csv", n_val, 7)):
        want = M.write_synthetic_csv(str(tmp_path / "want.csv"), rows, predictors, seed)
        assert (tmp_path / "out" / name).read_bytes() == open(want, "rb").read(), name
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["synthetic_train_rank0.csv", "synthetic_val_rank0.csv"]
    x, ev, du = data.collate([data.evaluation[i] for i in range(2)])
    want = M.ClinicalCsvDataset(str(tmp_path / "out" / "synthetic_val_rank0.csv"), predictors)
    assert x.shape == (2, 32) and np.array_equal(x[1].numpy(), want[1][0].numpy()) and np.array_equal(du[0].numpy(), want[0][2].numpy())


def test_every_rank_writes_its_own_training_csv(tmp_path):
    data, a, parser = _source(["--preop", "--classification", "--output_path", str(tmp_path), "--config", tiny_config(tmp_path)], rank=1, world=2)
    want = M.write_synthetic_csv(str(tmp_path / "want.csv"), 16, parser.predictors(a), 1001)
    assert (tmp_path / "synthetic_train_rank1.csv").read_bytes() == open(want, "rb").read()


@pytest.mark.parametrize("inference", [True, False])
def test_data_loc_is_what_inference_evaluates_and_training_trains_on(tmp_path, inference):
    predictors = [f"predictor{i}" for i in range(32)]
    x_csv = M.write_synthetic_csv(str(tmp_path / "x.csv"), 9, predictors, 5)
    data, a, _ = _source((["--inference"] if inference else []) + ["--preop", "--survival", "--data_loc", x_csv, "--output_path", str(tmp_path / "out"),
                                                                  "--config", tiny_config(tmp_path)])
    want = M.ClinicalCsvDataset(x_csv, predictors)
    assert len(data.evaluation) == len(data.train) == 9 and len(data.val) == 4
    for ds in (data.evaluation, data.train):
        assert all(np.array_equal(a.numpy(), b.numpy()) for i in (0, 8) for a, b in zip(ds[i], want[i]))
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["synthetic_val_rank0.csv"]         # (no training csv beside --data_loc)


def _radiomics_files(tmp_path):
    """A three-row table (uids 0, 1, 2) and the clinical csv that holds their targets."""
    rad = tmp_path / "rad.csv"
    rad.write_text("MRN,original_firstorder_Mean,original_shape_VoxelVolume\n" + "".join(f"{u},{u * 0.5 + 1},{u * 8.0 + 3}\n" for u in range(3)))
    return str(rad), M.write_synthetic_csv(str(tmp_path / "clinical.csv"), 3, [f"predictor{i}" for i in range(32)], 3)


@pytest.mark.parametrize("standardize", [True, False])
def test_radiomics_table_is_cut_into_the_split_uids(tmp_path, standardize):
    from mmnn_sts_amd.data.RadiomicsDatasets import SCALER_FILE
    rad, clin = _radiomics_files(tmp_path)
    (tmp_path / "train.txt").write_text("0\n2\n99\n")                  # (a uid the table does not hold is dropped)
    (tmp_path / "val.txt").write_text("1\n")
    cfg = tiny_config(tmp_path, radiomics={"standardize": standardize})
    base = ["--radiomics", "--survival", "--rad_loc", rad, "--data_loc", clin, "--output_path", str(tmp_path / "out"), "--config", cfg]
    data, a, _ = _source(base + ["--train_uid_location", str(tmp_path / "train.txt"), "--val_uid_location", str(tmp_path / "val.txt")])
    assert list(data.train.uids) == [0, 2] and list(data.val.uids) == [1] and data.evaluation is data.val
    assert data.collate is M.collate and data.train[0][0].shape == (2,)
    assert os.path.exists(tmp_path / "out" / SCALER_FILE) == standardize
    # without the two files: the seeded split of `split_uids`
    data, a, _ = _source(base + ["--train_uid_location", str(tmp_path / "none"), "--val_uid_location", str(tmp_path / "none")])
    train, val = M.split_uids([0, 1, 2], a, a.seed)
    assert (list(data.train.uids), list(data.val.uids)) == (train, val) and len(train) == 2 and len(val) == 1
    # two ranks share the training uids out and both evaluate the validation uids
    shard, _, _ = _source(base + ["--train_uid_location", str(tmp_path / "train.txt"), "--val_uid_location", str(tmp_path / "val.txt")], rank=1, world=2)
    assert list(shard.train.uids) == [2] and list(shard.val.uids) == [1]


def test_inference_needs_the_scaler_of_the_training_run(tmp_path):
    from mmnn_sts_amd.data.RadiomicsDatasets import SCALER_FILE
    rad, clin = _radiomics_files(tmp_path)
    argv = ["--inference", "--radiomics", "--survival", "--rad_loc", rad, "--data_loc", clin, "--output_path", str(tmp_path / "out"), "--config",
            tiny_config(tmp_path)]
    with pytest.raises(SystemExit) as e:
        _source(argv)
    assert str(e.value) == (f"--inference --radiomics reads the scaler the training run wrote: {tmp_path / 'out' / SCALER_FILE} is missing (same "
                            "--output_path, or `Radiomics: standardize: false`)")


def test_a_clinical_csv_beside_synthetic_images_is_refused(tmp_path):
    with pytest.raises(SystemExit) as e:
        _source(["--images", "--survival", "--data_loc", str(tmp_path / "x.csv"), "--output_path", str(tmp_path)])
    assert str(e.value) == ("clinical csv + image loaders need --image_loc (NIfTI patient directories) and --key_loc; run without --data_loc for "
                            "synthetic patients")
