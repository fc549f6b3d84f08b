"""White-box parity of the HIP DenseNet backbone (forward intermediates, running statistics, every parameter
gradient) against the CPU oracle on the same synthetic inputs.  fp32; tolerances written per check."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle import synth
from tests._util import rel_err, synth_sd

pytestmark = pytest.mark.gpu

CASES = [
    # (in_ch, block_config, (D,H,W), N)
    (2, (6, 12, 24, 16), (64, 64, 64), 2),
    (1, (6, 12, 24, 16), (64, 64, 64), 2),
    (2, (2, 2, 2), (40, 36, 44), 3),        # ragged, non power-of-two extents; odd remainders in every pool
    (2, (6, 12, 4), (64, 64, 64), 1),       # TinyDensenet layout, single sample
    (3, (2, 2), (40, 44, 48), 2),           # stem kernels are instantiated per input-channel count (csrc/stem.hip): odd count, no channel pairing
    (4, (2, 2), (36, 40, 44), 2),           # four channels: two LDS buffers of the conv0 forward at the 160 KB limit
]


def _run_case(in_ch, blocks, dhw, n, full=True):
    """Truth = the oracle evaluated in fp64 (the fp32 oracle itself is only within ~3e-5 of it at 64^3, see
    DESIGN.md "Tolerances"); bar = 1e-4 relative (north star) on every intermediate, the output and the running
    statistics; gradients: per-tensor L2 error <= 1e-3*|g| + 1e-5*|g_all| (several gradients are analytically 0).
    `full=False`: extents whose last block has a single voxel per sample -- two-sample batch norm is ill-conditioned
    there (fp32 and fp64 oracles disagree by >10 %), so only the blocks before it are compared."""
    from tests._native import NativeBackbone, backbone_run_keys
    cfg = R.DenseNetCfg(in_channels=in_ch, block_config=blocks)
    sch = R.densenet_schema(cfg)
    x = torch.from_numpy(synth.uniform(f"bb/{n}x{in_ch}x{dhw}", (n, in_ch) + dhw))
    nb = NativeBackbone(cfg, n, *dhw)
    flat, run = nb.flatten(synth_sd(sch, "densenet."))
    xg = x.cuda()
    out = nb.forward(flat, run, xg, training=True)
    torch.cuda.synchronize()
    # fp64 oracle taking the SAME ReLU branches as the device (ReLU'(0) is a convention; near-zero pre-activations would
    # otherwise make any two fp32 implementations disagree by percents in block 4, where a channel has N*V = 16 samples)
    masks = nb.relu_masks(flat) if full else None
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v)
          for k, v in synth_sd(sch, "densenet.").items()}
    taps = {}
    h = R.densenet_backbone(sd, x.double(), cfg, True, taps=taps, relu_masks=masks)
    cot = torch.from_numpy(synth.uniform("bb/cot", tuple(h.shape)))
    if full:
        (h * cot.double()).sum().backward()
    errs = {}
    c0 = taps["conv0"]
    errs["conv0"] = rel_err(nb.region("conv0", tuple(c0.shape)).cpu().numpy(), c0.detach().numpy())
    nblk = len(blocks) if full else len(blocks) - 1
    for b in range(nblk):
        ref = taps[f"block{b + 1}"].detach()
        errs[f"block{b + 1}"] = rel_err(nb.region("x", tuple(ref.shape), b).cpu().numpy(), ref.numpy())
    if full:
        errs["norm5"] = rel_err(out.cpu().numpy(), h.detach().numpy())
    assert torch.isfinite(out).all()
    for k, e in errs.items():
        assert e < 1e-4, (k, errs)
    if not full:
        return errs, None
    got_run = nb.unflatten(run.cpu(), backbone_run_keys(sch))
    for k, v in got_run.items():
        assert rel_err(v.numpy(), sd[k].detach().numpy()) < 1e-4, k
    g = nb.backward(flat, xg, cot.cuda())
    torch.cuda.synchronize()
    got = nb.unflatten(g.cpu())
    gl2 = float(torch.sqrt(sum((sd[k].grad ** 2).sum() for k in got)))
    worst = (0.0, "")
    bad = []
    for k, v in got.items():
        ref = sd[k].grad
        err = float((v.double() - ref).norm())
        tol = 1e-3 * float(ref.norm()) + 1e-5 * gl2
        worst = max(worst, (err / tol, k))
        if err > tol:
            bad.append((k, err, float(ref.norm()), float(v.double().norm())))
    assert not bad, (len(bad), len(got), gl2, bad[:3], bad[-12:])
    return errs, worst


@pytest.mark.parametrize("in_ch,blocks,dhw,n", CASES)
def test_backbone_forward_backward(in_ch, blocks, dhw, n):
    errs, worst = _run_case(in_ch, blocks, dhw, n)
    print("forward rel errors", errs, "worst gradient (err/tol, name)", worst)


# Tile-instantiation matrix.  Tile shapes are picked from the extent (csrc/fprop_dispatch.hpp: `dispatch`, csrc/wgrad.hip:
# `wg3_tile`, `wg1_wc`), so every branch needs an extent of its own.  Block-1 extents of the cases (block 2 = half of it):
#   20^3 (N=4)    W > 16: wave-specialised conv2 forward <27,..,2,4,32,true>, KC=2 conv2 data-grad <27,PRO_GRAD,..,1,4,32>,
#                 wgrad3<1,2,32>; 252 voxel tiles -> 128-wide 1x1x1 tile for conv1 forward / data-grad; block 2: W = 10 tiles
#   6x10x17       ragged W just above the 16 boundary, odd rows (no 16-byte staging: scalar path of the W > 16 tiles)
#   4x6x33        W = 33: one full 32-wide tile + a 1-voxel remainder tile in every row
#   12x12x40      64-wide 1x1x1 tile (blocks_a < 192 <= blocks_b) incl. the PRO_NONE transition conv at 20x6x6
#   8x10x18       a one-layer block 1: conv2 weight gradient as a batch of one, conv1 weight gradient on the unbatched kernel
# The BASELINE extents themselves (32^3 .. 4^3 at N = 2) run in test_baseline_config3_backbone_128.
MATRIX = [
    (2, (2, 2), (80, 80, 80), 4),
    (2, (2, 2), (24, 40, 66), 2),
    (1, (2, 2), (16, 24, 130), 2),
    (2, (3, 2), (48, 48, 160), 2),
    (2, (1, 3), (32, 40, 72), 2),
]


@pytest.mark.parametrize("in_ch,blocks,dhw,n", MATRIX)
def test_backbone_tile_matrix(in_ch, blocks, dhw, n):
    errs, worst = _run_case(in_ch, blocks, dhw, n)
    print("forward rel errors", errs, "worst gradient (err/tol, name)", worst)


def test_baseline_config3_backbone_128():
    """The backbone of BASELINE configs[2] at its own size (2 x 2 x 128^3): every intermediate, the running statistics and all
    364 backbone gradients against the fp64 oracle -- this is the extent whose W > 16 tiles the benchmark dispatches to."""
    errs, worst = _run_case(2, (6, 12, 24, 16), (128, 128, 128), 2)
    print("forward rel errors", errs, "worst gradient (err/tol, name)", worst)


def test_baseline_config2_backbone_128():
    """BASELINE configs[1]: single-channel (t1) volumes, 2 x 1 x 128^3."""
    errs, worst = _run_case(1, (6, 12, 24, 16), (128, 128, 128), 2)
    print("forward rel errors", errs, "worst gradient (err/tol, name)", worst)


def test_backbone_minimum_extent():
    """32^3 is the smallest legal input: every block must run (1x1x1 voxels in block 4)."""
    _run_case(2, (6, 12, 24, 16), (32, 32, 32), 2, full=False)


def test_backbone_accumulate_and_eval():
    from tests._native import NativeBackbone
    cfg = R.DenseNetCfg(in_channels=2, block_config=(2, 2))
    sch = R.densenet_schema(cfg)
    sd = synth_sd(sch, "densenet.")
    x = torch.from_numpy(synth.uniform("bb/acc", (2, 2, 24, 24, 24)))
    with torch.no_grad():
        ref = R.densenet_backbone(sd, x, cfg, False)
    nb = NativeBackbone(cfg, 2, 24, 24, 24)
    flat, run = nb.flatten(synth_sd(sch, "densenet."))
    run0 = run.clone()
    out = nb.forward(flat, run, x.cuda(), training=False)
    assert rel_err(out.cpu().numpy(), ref.numpy()) < 2e-5
    assert torch.equal(run, run0)                      # eval never touches the running statistics
    out = nb.forward(flat, run, x.cuda(), training=True)
    cot = torch.ones_like(out)
    g1 = nb.backward(flat, x.cuda(), cot).clone()
    g2 = nb.backward(flat, x.cuda(), cot, accumulate=True, grad=g1.clone())
    torch.cuda.synchronize()
    assert rel_err(g2.cpu().numpy(), (2 * g1).cpu().numpy()) < 1e-6
    # run-to-run: statistics are fp64-accumulated, weight gradients are slab sums (no fp32 atomics on tensors)
    out2 = nb.forward(flat, run, x.cuda(), training=True)
    g3 = nb.backward(flat, x.cuda(), cot)
    torch.cuda.synchronize()
    assert rel_err(g3.cpu().numpy(), g1.cpu().numpy()) < 1e-5 and rel_err(out2.cpu().numpy(), out.cpu().numpy()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("in_ch", [1, 2])
def test_backbone_repeated_calls_are_bit_identical(in_ch):
    """One plan, many calls: every forward / backward of the same inputs must reproduce the first bit for bit, whatever ran
    before it (the kernels keep no state between calls and never read LDS or workspace words they did not write)."""
    from tests._native import NativeBackbone
    cfg = R.DenseNetCfg(in_channels=in_ch)
    n, s = 2, 64
    nb = NativeBackbone(cfg, n, s, s, s)
    flat, run = nb.flatten(synth_sd(R.densenet_schema(cfg), "densenet."))
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(n, in_ch, s, s, s, device="cuda", generator=g)
    cot = torch.randn(nb.out_shape, device="cuda", generator=g)
    ref_o = ref_g = None
    for op in "FFBFBBFFB":
        if op == "F":
            o = nb.forward(flat, run.clone(), x, True, seed=1)
            assert torch.isfinite(o).all()
            if ref_o is None:
                ref_o = o
            assert torch.equal(o, ref_o), f"forward deviates by {float((o - ref_o).abs().max())}"
        else:
            gr = nb.backward(flat, x, cot, seed=1)
            assert torch.isfinite(gr).all()
            if ref_g is None:
                ref_g = gr
            assert torch.equal(gr, ref_g), f"backward deviates by {float((gr - ref_g).abs().max())}"


@pytest.mark.parametrize("mode", ["0"])
def test_bf16x3_switch_positions_keep_parity(mode):
    """The suite runs with the default kernel selection (conv2 forward / data gradient of extents wider than 16 voxels on three-piece bf16
    MFMAs, csrc/conv3_bf16x3.hip).  The switch is read once per process, so the other position runs in a fresh one: MMNN_BF16X3=0 (the
    fp32-MFMA kernels for every extent) must pass the same tile-matrix parity (ragged W = 17 / 33 included) against the fp64 oracle at the
    same tolerances."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMNN_BF16X3=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "tile_matrix"], env=env, cwd=root,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"{len(MATRIX)} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
