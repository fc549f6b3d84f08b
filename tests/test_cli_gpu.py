"""main.py as a fresh process for the BASELINE configs it serves (tiny synthetic sizes): exit code, saved checkpoint reloads
into a freshly built model with strict=True, attention maps written."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_run = functools.partial(run_main, limit_s=900)
_run_ranks = functools.partial(run_main, limit_s=900, world=2)        # two ranks sharing the one card over gloo


def test_config0_preop_classification(tmp_path):
    """BASELINE configs[0]: `--preop --classification`, 32-feature x 64-patient csv -> standalone MLP, pos-weighted BCE."""
    from mmnn_sts_amd.models.mlp import MLP
    log = _run(["--preop", "--classification", "--epochs", "2", "--synthetic_patients", "64", "--config", tiny_config(tmp_path)], tmp_path)
    assert "saved new best metric model" in log and "epoch 2/2" in log
    rows = np.loadtxt(tmp_path / "synthetic_train_rank0.csv", delimiter=",", skiprows=1)
    assert rows.shape == (64, 1 + 32 + 4)
    MLP(32, 2, 12).load_state_dict(torch.load(tmp_path / "model.pth"), strict=True)
    MLP(32, 2, 12).load_state_dict(torch.load(tmp_path / "final_model.pth"), strict=True)


def test_config1_images_survival_t1(tmp_path):
    """BASELINE configs[1]: `--images --survival`, single-channel volumes, unimodal DenseNet."""
    from mmnn_sts_amd.models.densenet import TinyDensenet
    log = _run(["--images", "--survival", "--epochs", "2", "--synthetic_patients", "6", "--synthetic_size", "32",
                "--config", tiny_config(tmp_path, "t1", 1)], tmp_path)
    assert "epoch 2/2" in log
    m = TinyDensenet(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, dropout_prob=0.2)
    m.load_state_dict(torch.load(tmp_path / "best_surv_model.pth"), strict=True)


def test_config2_fusion_blend_then_config4_gradcam(tmp_path):
    """BASELINE configs[2] then configs[4]: train the fusion model with the GradientBlender (weights updated after epoch 2), then
    reload the checkpoint for Grad-CAM inference."""
    from mmnn_sts_amd.models.densenet import TinyDensenet
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    cfg = tiny_config(tmp_path)
    log = _run(["--images", "--preop", "--survival", "--blend", "--blend_update_interval", "2", "--epochs", "2", "--synthetic_patients", "6",
                "--synthetic_size", "32", "--config", cfg], tmp_path)
    assert "Completed updating gradient blender weights" in log
    hist = np.loadtxt(tmp_path / "gblend_weights_history.csv", delimiter=",", ndmin=2)
    assert hist.shape == (1, 3) and abs(hist.sum() - 1.0) < 1e-5
    img = TinyDensenet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.2)
    MultiModalModel(img, [f"p{i}" for i in range(32)], 2, 12, blend=True).load_state_dict(torch.load(tmp_path / "best_surv_model.pth"), strict=True)
    log = _run(["--inference", "--images", "--preop", "--survival", "--weights", str(tmp_path / "best_surv_model.pth"), "--synthetic_patients", "8",
                "--synthetic_size", "32", "--config", cfg], tmp_path)
    assert "All C-indexes" in log
    m = np.load(tmp_path / "attention_maps" / "patient0_att_map.npy")
    assert m.shape == (32, 32, 32) and np.isfinite(m).all() and m.min() >= 0.0 and m.max() <= 1.0 + 1e-6


def test_bench_two_ranks_at_baseline_extent(tmp_path):
    """BASELINE configs[3] rehearsal on ONE card: `bench.py --gpus 2 --size 128` starts its two ranks itself, the
    ranks share the card over gloo (RCCL needs one device per rank), gradients are all-reduced per dense block from inside the backward.
    The JSON line must report both ranks, a finite throughput and the overlapped schedule."""
    import json
    env = dict(os.environ, MMNN_DIST_BACKEND="gloo", MMNN_POISON_LDS="0", MMNN_POISON_WS="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--size", "128", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-roofline"], env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == d["ranks_seen"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 4
    assert d["config"]["allreduce"].startswith("per dense block") and d["scaling"] == "weak"
    assert np.isfinite(d["value"]) and d["value"] > 0 and d["steps"] == 2


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run prints the headline line without the --full legs, and `--dump-outputs DIR` writes the last timed
    step's risk scores, loss, updated parameters and running statistics as float32 .npy files (at most 64 MB in all) that agree between
    two runs of the same command (seeded inputs)."""
    import json
    from bench import build_model
    env = dict(os.environ, MMNN_POISON_LDS="0", MMNN_POISON_WS="0")
    dumps = []
    for run in range(2):
        out = tmp_path / f"out{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == 3 and d["higher_is_better"] is True and d["dtype"] == "f32" and d["unit"].startswith("volumes/s")
        assert np.isfinite(d["ms_per_step"]) and d["ms_per_step"] > 0 and abs(d["value"] - 2e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert "roofline" not in d and "cpu_baseline" not in d
        files = sorted(p.name for p in out.iterdir())
        assert files == ["loss.npy", "parameters.npy", "risk_scores.npy", "running_stats.npy"]
        assert sum(p.stat().st_size for p in out.iterdir()) <= 64 * 2 ** 20
        a = {f[:-4]: np.load(out / f) for f in files}
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
        assert a["parameters"].size == sum(p.numel() for p in build_model("cpu").parameters()) and a["loss"].shape == (1,)
        dumps.append(a)
    for k in dumps[0]:
        np.testing.assert_allclose(dumps[1][k], dumps[0][k], rtol=1e-3, atol=1e-5, err_msg=k)


def test_two_rank_survival_blend_and_classification(tmp_path):
    """The CLI's data-parallel paths on two ranks: survival + GradientBlender (accumulation windows whose last backward arms the overlapped
    reducer, blender update on gathered predictions, rank 0 saves) and classification (broadcast, all-reduce before every
    optimizer step, checkpoints written by rank 0 only)."""
    from mmnn_sts_amd.models.densenet import TinyDensenet
    from mmnn_sts_amd.models.mlp import MLP
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    cfg = tiny_config(tmp_path)
    a = tmp_path / "surv"; a.mkdir()
    log = _run_ranks(["--images", "--preop", "--survival", "--blend", "--blend_update_interval", "1", "--epochs", "1", "--synthetic_patients", "6",
                      "--synthetic_size", "32", "--config", cfg], a)
    assert "Completed updating gradient blender weights" in log and log.count("saved new best metric model") == 1      # rank 0 only
    img = TinyDensenet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.2)
    MultiModalModel(img, [f"p{i}" for i in range(32)], 2, 12, blend=True).load_state_dict(torch.load(a / "best_surv_model.pth"), strict=True)
    b = tmp_path / "cls"; b.mkdir()
    log = _run_ranks(["--preop", "--classification", "--epochs", "2", "--synthetic_patients", "16", "--config", cfg], b)
    assert log.count("epoch 2/2") == 1                                                                                  # rank 0 logs
    MLP(32, 2, 12).load_state_dict(torch.load(b / "final_model.pth"), strict=True)
    assert sorted(p.name for p in b.glob("synthetic_train_rank*.csv")) == ["synthetic_train_rank0.csv", "synthetic_train_rank1.csv"]
