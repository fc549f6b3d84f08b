"""Pre-split operands of the wide conv2 kernels (csrc/conv3_bf16x3.hip, csrc/bf16x3.hpp): the split passes' three bf16 planes and the
pre-split weight panels (pack kinds 5 / 6), checked against torch restatements, at the ragged extents W = 17 / 33 and at 32^3."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle import synth

from tests._native import NativeBackbone

pytestmark = pytest.mark.gpu

# (input extent, N): block 1 at 6x10x17, 4x6x33 and 16^3 x 32 (W > 16: the bf16x3 kernels); block 2 is narrow and stays on fprop_kernel
CASES = [((24, 40, 66), 2), ((16, 24, 130), 2), ((64, 64, 128), 1)]


def _setup(dhw, n, seed_name, dropout=0.0):
    cfg = R.DenseNetCfg(in_channels=2, block_config=(2, 2))
    nb = NativeBackbone(cfg, n, *dhw, dropout=dropout)
    sch = nb.schema
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(sch, seed_name).items()}
    flat, run = nb.flatten(sd)
    x = torch.from_numpy(synth.uniform(seed_name + "x", (n, 2, *dhw))).cuda()
    return cfg, nb, flat, run, x


def _block1_dims(dhw):
    d0 = [(s - 1) // 2 + 1 for s in dhw]
    return [(s - 1) // 2 + 1 for s in d0]


def _pieces(nb, n, c, v):
    """The plane scratch as (hi, mid, lo), each (n, c, v) in fp64, channel c = 8 * group + k."""
    raw = nb.region("x3", (3, n, c // 8, v, 8), dtype=torch.bfloat16).double()
    raw = raw.permute(0, 1, 2, 4, 3).reshape(3, n, c, v)
    return raw[0], raw[1], raw[2]


def _check_split(hi, mid, lo, ref):
    """hi / mid / lo are the round-to-nearest bf16 pieces of one fp32 value close to `ref` (fp64)."""
    x = (hi + mid + lo).float()
    scale = float(ref.abs().max())
    assert scale > 0
    err = float((hi + mid + lo - ref).abs().max())
    assert err <= 2e-6 * scale, (err, scale)
    # every piece is the bf16 rounding of what the pieces before it left over (a tie can only move a value off by its last bit)
    assert float((x.to(torch.bfloat16).double() != hi).double().mean()) < 1e-3
    assert float((((x.double() - hi).float()).to(torch.bfloat16).double() != mid).double().mean()) < 1e-3
    assert bool(((mid.abs() <= hi.abs() * 2.0 ** -8 + 1e-30) | (hi == 0)).all())
    assert bool(((lo.abs() <= mid.abs() * 2.0 ** -8 + 1e-30) | (mid == 0)).all())
    assert bool(((hi == 0) == (x == 0)).all())


@pytest.mark.parametrize("dhw,n", CASES)
def test_forward_planes_are_split_bnrelu(dhw, n):
    cfg, nb, flat, run, x = _setup(dhw, n, "c3split.")
    if nb.L.mmnn_densenet_ws_offset(nb.plan, b"x3", 0, 0) < 0:
        pytest.skip("three-piece bf16 kernels switched off (MMNN_BF16X3=0)")
    nb.forward(flat, run, x, training=True)
    torch.cuda.synchronize()
    D, H, W = _block1_dims(dhw)
    V = D * H * W
    mid_c = cfg.bn_size * cfg.growth_rate
    last = cfg.block_config[0] - 1            # the planes hold the last wide conv2 forward: block 1's last layer
    t1 = nb.region("t1", (n, mid_c, V), 0, last).double().cpu()
    p = nb.unflatten(flat.cpu())
    g = p[f"backbone.denseblock1.denselayer{last + 1}.layers.norm2.weight"].double()
    b = p[f"backbone.denseblock1.denselayer{last + 1}.layers.norm2.bias"].double()
    mean = t1.mean(dim=(0, 2))
    var = t1.var(dim=(0, 2), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    ref = torch.relu(t1 * (g * rstd)[None, :, None] + (b - mean * g * rstd)[None, :, None])
    hi, mi, lo = (t.cpu() for t in _pieces(nb, n, mid_c, V))
    _check_split(hi, mi, lo, ref)
    # ReLU zeros stay exact zeros in all three pieces
    assert bool(((hi != 0) | ((mi == 0) & (lo == 0))).all())


@pytest.mark.parametrize("dhw,n", CASES[:2])
def test_weight_panels_are_split_weights(dhw, n):
    cfg, nb, flat, run, x = _setup(dhw, n, "c3panel.")
    if nb.L.mmnn_densenet_ws_offset(nb.plan, b"pk_c2f3", 0, 0) < 0:
        pytest.skip("three-piece bf16 kernels switched off (MMNN_BF16X3=0)")
    nb.forward(flat, run, x, training=True)
    torch.cuda.synchronize()
    mid_c, gr = cfg.bn_size * cfg.growth_rate, cfg.growth_rate
    p = nb.unflatten(flat.cpu())
    for l in range(cfg.block_config[0]):
        w = p[f"backbone.denseblock1.denselayer{l + 1}.layers.conv2.weight"].reshape(gr, mid_c, 27).double()   # [m][c][tap]
        f = nb.region("pk_c2f3", (3, 27, mid_c // 8, gr, 8), 0, l, dtype=torch.bfloat16).double().cpu()
        f = f.sum(0).permute(2, 1, 3, 0).reshape(gr, mid_c, 27)                          # [m][c8][k][tap] -> [m][c][tap]
        assert float((f - w).abs().max()) <= 1e-7 * float(w.abs().max())
        bw = nb.region("pk_c2b3", (3, 27, gr // 8, mid_c, 8), 0, l, dtype=torch.bfloat16).double().cpu()
        hi = bw[0].permute(1, 3, 2, 0).reshape(gr, mid_c, 27).flip(-1)                   # [tap][m8][c][k] -> [m][c][26 - tap]
        assert torch.equal(hi, w.float().to(torch.bfloat16).double())
        bw = bw.sum(0).permute(1, 3, 2, 0).reshape(gr, mid_c, 27).flip(-1)
        assert float((bw - w).abs().max()) <= 1e-7 * float(w.abs().max())


@pytest.mark.parametrize("dhw,n", CASES[:2])
def test_dgrad_planes_and_repeatability(dhw, n):
    cfg, nb, flat, run, x = _setup(dhw, n, "c3dgrad.")
    if nb.L.mmnn_densenet_ws_offset(nb.plan, b"x3", 0, 0) < 0:
        pytest.skip("three-piece bf16 kernels switched off (MMNN_BF16X3=0)")
    cot = torch.from_numpy(synth.uniform("c3dgrad.cot", nb.out_shape)).cuda()
    D, H, W = _block1_dims(dhw)
    V = D * H * W
    outs = []
    for _ in range(2):
        run_i = run.clone()
        out = nb.forward(flat, run_i, x, training=True)
        g = nb.backward(flat, x, cot)
        torch.cuda.synchronize()
        planes = nb.region("x3", (3, n, cfg.growth_rate // 8, V, 8), dtype=torch.bfloat16).clone()
        outs.append((out.clone(), g.clone(), run_i, planes))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)                 # repeated calls: bit-identical outputs, gradients, running statistics and planes
    hi, mi, lo = (t.cpu() for t in _pieces(nb, n, cfg.growth_rate, V))
    # the data-gradient operand of block 1's first layer (the last wide conv2 data gradient of the backward): a well-formed split
    s = hi + mi + lo
    assert float(s.abs().max()) > 0
    _check_split(hi, mi, lo, s)


@pytest.mark.parametrize("dhw,n", CASES[:2])
def test_dgrad_planes_with_dropout(dhw, n):
    """p = 0.2: the split pass folds the layer's dropout scale into the batch-norm backward coefficients (conv3_split_bnbwd_kernel, code
    of its own).  The planes of a dropped (n, c) channel are exact zeros, every kept channel has a non-zero element, and hi + mid + lo is
    scale * (p G + q X + r) rebuilt in fp64 from the gradient / activation regions and the fp64 statistics (st_x: sums of X and X^2,
    s_x: sums of G and G * xhat; NREP = 8 replica rows of `ctot` channels each, unused rows zero)."""
    from tests._util import channel_drop_mask
    seed, p = 0xD1B54A32D192ED03, 0.2
    cfg, nb, flat, run, x = _setup(dhw, n, "c3drop.", dropout=p)
    if nb.L.mmnn_densenet_ws_offset(nb.plan, b"x3", 0, 0) < 0:
        pytest.skip("three-piece bf16 kernels switched off (MMNN_BF16X3=0)")
    cot = torch.from_numpy(synth.uniform("c3drop.cot", nb.out_shape)).cuda()
    nb.forward(flat, run, x, training=True, seed=seed)
    nb.backward(flat, x, cot, seed=seed)
    torch.cuda.synchronize()
    D, H, W = _block1_dims(dhw)
    V = D * H * W
    gr, c0 = cfg.growth_rate, cfg.init_features
    ctot = c0 + cfg.block_config[0] * gr
    hi, mi, lo = (t.cpu() for t in _pieces(nb, n, gr, V))          # the last wide data gradient of the backward: block 1, layer 1 (id 0)
    mask = torch.from_numpy(channel_drop_mask(seed, 0, n, gr, p)).double()
    assert bool((mask == 0).any()) and bool((mask != 0).any())
    alive = ((hi != 0) | (mi != 0) | (lo != 0)).any(dim=2)
    assert torch.equal(alive, mask != 0)
    G = nb.region("g", (n, ctot, V), 0).double().cpu()[:, c0:c0 + gr]
    X = nb.region("x", (n, ctot, V), 0).double().cpu()[:, c0:c0 + gr]
    st = nb.region("st_x", (2, 8, ctot), 0, dtype=torch.float64).cpu().sum(1)[:, c0:c0 + gr]
    sg = nb.region("s_x", (2, 8, ctot), 0, dtype=torch.float64).cpu().sum(1)[:, c0:c0 + gr]
    assert torch.isfinite(st).all() and torch.isfinite(sg).all()
    cnt = float(n * V)
    mean = st[0] / cnt
    rstd = 1.0 / torch.sqrt((st[1] / cnt - mean * mean).clamp_min(0) + 1e-5)
    m1, m2 = sg[0] / cnt, sg[1] / cnt
    # the statistics are the device's own; pin them to the data they were taken of before using them
    assert float((mean - X.mean(dim=(0, 2))).abs().max()) <= 1e-6 * float(X.abs().max())
    pc, qc, rc = rstd, -rstd * rstd * m2, rstd * rstd * m2 * mean - rstd * m1
    ref = mask[:, :, None] * (pc[None, :, None] * G + qc[None, :, None] * X + rc[None, :, None])
    print("planes against the fp64 rebuild: max abs err / max", float((hi + mi + lo - ref).abs().max() / ref.abs().max()))
    _check_split(hi, mi, lo, ref)


def test_training_step_on_split_operands_matches_oracle():
    """A training forward + backward whose block 1 runs on the pre-split kernels (W = 33) against the fp64 oracle, at the tolerances of
    tests/test_backbone_gpu.py."""
    from tests.test_backbone_gpu import _run_case
    _run_case(1, (2, 2), (16, 24, 130), 2)
