"""What the tests that drive a command line share: the fresh-process runner (main.py alone or under torch.distributed.run, or any other
python command line of the package) and the smallest config those command lines train on."""
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "main.py")


def run_python(argv, cwd, *, limit_s, expect_ok=True, env=None):
    """`python *argv` in a fresh process in `cwd`, poison switches off, the package importable, under its own `timeout -k 10 limit_s`
    -> its combined output; a status other than 0 fails the test with the end of that output.  `expect_ok=False`: the completed
    process, whatever its status.  `env`: variables laid over the environment (None removes one)."""
    full = dict(os.environ, MMNN_POISON_LDS="0", MMNN_POISON_WS="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k, v in (env or {}).items():
        if v is None:
            full.pop(k, None)
        else:
            full[k] = v
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit_s), sys.executable, *argv], cwd=str(cwd), env=full, capture_output=True, text=True)
    if not expect_ok:
        return r
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def run_main(args, out, *, limit_s, world=1, expect_ok=True, env=None):
    """`main.py --output_path out *args` through `run_python`, in `out`.  `world` > 1: under torch.distributed.run on a free port, the
    ranks sharing the one card over gloo (on an 8-GPU node the same command runs over RCCL)."""
    argv = [MAIN, "--output_path", str(out), *args]
    if world > 1:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        argv = ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(port)] + argv
        env = dict({"MMNN_DIST_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "OMP_NUM_THREADS": "2", "RANK": None, "WORLD_SIZE": None,
                    "LOCAL_RANK": None}, **(env or {}))
    return run_python(argv, out, limit_s=limit_s, expect_ok=expect_ok, env=env)


def tiny_config(tmp_path, modality="t1t2", in_channels=2, *, data=None, radiomics=None, **image_model):
    """Writes the smallest config the command lines train on -> its path.  `data` / `radiomics`: the `Data:` / `Radiomics:` section, if
    any; `image_model`: further overrides of the `ImageModel:` keys."""
    import yaml
    cfg = {"ImageModel": dict({"name": "tinydensenet", "modality": modality, "feature_layers": 12, "num_classes": 2, "spatial_dims": 3,
                               "in_channels": in_channels, "dropout_prob": 0.2}, **image_model),
           "ClinicalModel": {"NUM_PREDICTORS": 32, "PRE_OP_PREDICTORS": [], "POST_OP_PREDICTORS": []},
           "Hyperparameters": {"momentum": 0.9, "weight_decay": 1e-4, "train_batch_size": 2, "seed": 42, "class_frequencies": [0.4, 0.55]}}
    for name, section in (("Data", data), ("Radiomics", radiomics)):
        if section is not None:
            cfg[name] = dict(section)
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)
