"""The data gradients of the HIP DenseNet backward, voxel by voxel: every workspace region of the backward (and the two forward regions
nothing else compares) against the fp64 oracle in the max-norm, at the extents that reach each tile branch.  What the regions mean and how
the reference is built: tests/_backward_taps.py; that the reference is right: tests/test_backbone_backward_taps_cpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from tests import _backward_taps as T
from tests._util import backbone_drop_masks, synth_sd
from oracle import restatement as R
from oracle import synth

pytestmark = pytest.mark.gpu

SEED_A = 0x9E3779B97F4A7C15        # the seeds of tests/test_backbone_gpu.py
SEED_B = 20260213


def _run(name, dropout=0.0, seed=0, options=()):
    """Training forward, then the backward as a walk of single-block calls with the regions copied between the calls
    (tests/_native.py: backward_walk).  The fp64 oracle takes the device's ReLU branches, pool winners and dropout masks, as
    tests/test_backbone_gpu.py::_run_case does.  Every region <= 1e-4 max-norm relative (T.BAR: the bar of the forward intermediates), the
    fp64 sums S1 / S2 <= 1e-4 of max |S| per block; the walk's gradient buffer equals the single call's bit for bit."""
    from tests._native import NativeBackbone
    in_ch, blocks, dhw, n = T.CASES[name]
    cfg, x = T.case_inputs(in_ch, blocks, dhw, n)
    nb = NativeBackbone(cfg, n, *dhw, dropout=dropout)
    for opt, value in options:
        nb.set_option(opt, value)
    if os.environ.get("MMNN_BF16X3") == "0":          # the switch took effect: no bf16 plane scratch in the plan
        assert nb.L.mmnn_densenet_ws_offset(nb.plan, b"x3", 0, 0) < 0
    flat, run = nb.flatten(synth_sd(R.densenet_schema(cfg), "densenet."))
    xg = x.cuda()
    out = nb.forward(flat, run, xg, training=True, seed=seed)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    drop = None
    if dropout > 0:
        drop = backbone_drop_masks(cfg, seed, n, dropout)
        alive = nb.device_drop_masks()
        for k, m in drop.items():          # dropped channels are exact zeros on the device, where the restated masks say so
            assert bool((m == 0).any()) and bool((m != 0).any()), k
            assert torch.equal(alive[k], m != 0), k
    masks, pool = nb.relu_masks(flat), nb.pool_taps()
    got = {k: v.cpu() for k, v in nb.forward_taps().items()}
    sd, taps, h = T.oracle_run(cfg, x, relu_masks=masks, drop_masks=drop, pool_taps=pool)
    assert float(taps["pool_gap"].max()) <= 1e-4 * float(taps["stem"].detach().abs().max())
    if drop is not None:                   # ... and in the reference's gradient of every conv2 output, dz2's upstream
        for k, m in drop.items():
            assert not bool(taps[k + "y"].grad[m == 0].any()), k
    ref = T.build_reference(cfg, sd, taps, masks)
    cot = torch.from_numpy(synth.uniform("bb/cot", tuple(h.shape))).cuda()
    grad, snap = nb.backward_walk(flat, xg, cot, seed=seed)
    torch.cuda.synchronize()
    got.update({k: v.cpu() for k, v in snap.items()})
    assert set(got) == set(ref), set(got) ^ set(ref)
    res = T.compare(got, ref)
    assert set(res) == set(T.KINDS)
    tag = name + (f" p={dropout}" if dropout else "") + "".join(f" {o}={v}" for o, v in options)
    for kind in T.KINDS:
        e, key, idx = res[kind]
        print(f"{tag}: {kind:4s} device {e:.2e} (fp32 floor {T.FLOOR[name][kind]:.1e}) worst {key} at {idx}")
    for kind in T.KINDS:
        e, key, idx = res[kind]
        assert e <= T.BAR, (tag, kind, e, key, idx)
    single = nb.backward(flat, xg, cot, seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(grad, single), float((grad - single).abs().max())
    return res


@pytest.mark.parametrize("name", list(T.CASES))
def test_backward_taps_tile_matrix(name):
    _run(name)


def test_backward_taps_without_k_split():
    _run("ksplit", options=(("no_kz", 1),))


@pytest.mark.parametrize("name,seed", [("w17", SEED_A), ("narrow", SEED_B)])
def test_backward_taps_dropout(name, seed):
    _run(name, dropout=0.2, seed=seed)


def test_backward_taps_with_fp32_mfma_kernels():
    """MMNN_BF16X3=0 is read once per process: the W = 17 and W = 33 cases run in a fresh one, on the fp32-MFMA conv2 kernels."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMNN_BF16X3="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-k", "tile_matrix and (w17 or w33)"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
