"""Backward taps of the DenseNet backbone: what every workspace region of the backward holds, rebuilt from the oracle's retained
gradients (oracle/restatement.py: densenet_backbone(taps=)), and a max-norm comparator that names the worst voxel.

The regions (mmnn_densenet_ws_offset) and their meaning, each read off the kernel that writes it:

  dz2[b][l]  csrc/densenet.hip plan_backward_range: conv2 data gradient, PRO_GRAD prologue on (g_new, x_new), EPI_MASK_STORE epilogue
             with the ReLU branch of norm2 (csrc/fprop.hpp header).  = dL/d(norm2 output), zero where the ReLU is off.
             Reference: .grad of the tap "b{b}l{l}n2".
  g[b]       first written by consumer_bwd (csrc/elementwise.hip: norm5 stores gamma5 * dy; a transition stores gamma_t * mask *
             unpool(dap) / 8), then every conv1 data gradient adds gamma1 * z on its channels [0, cin) (EPI_MASK_ACCUM, z = masked
             gradient of the norm1 output).  BnBwd::gamma is null for these channels (csrc/common.hpp): G = dL/dxhat of the concat
             buffer with every consumer's gamma folded in.  Reference: sum over the norms that read the buffer of gamma * .grad(norm
             output) on the channels that norm sees.
  s_x[b]     S1 = sum G, S2 = sum G * xhat per concat channel (fp64 replicas, unused ones zero): the sums of BnBwd.
  dap        data gradient of the transition's 1x1x1 convolution wrt its input, the POOLED normalised activations (the device pools
             before it convolves; pool and 1x1x1 convolution commute).  Reference: transition weight transposed applied to
             .grad of "trans{b}".  One buffer for every transition: valid after the backward of block b + 1.
  dz0        csrc/stem.hip stem_pool_bwd_kernel: BN-backward of the first block's stem channels evaluated on the fly, routed to the
             winner of every pool window, times the ReLU branch of norm0.  = dL/d(norm0 output); norm0's own backward happens
             inside the conv0 weight gradient.  Reference: .grad of the tap "norm0".
  t1[b][l]   conv1 output (forward).  Reference: tap "b{b}l{l}t1".
  ap[b]      avg-pool of ReLU(transition norm) (forward).  Reference: avg_pool3d of the masked tap "t{b}n".

Keys of a reference / snapshot dict: ("dz2", b, l), ("g", b), ("s_x", b), ("dap", b), ("dz0",), ("t1", b, l), ("ap", b), b and l 0-based;
("dap", b) and ("ap", b) belong to the transition behind block b.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import restatement as R
from oracle import synth
from tests._util import synth_sd

BAR = 1e-4          # max-norm relative, the bar of the forward intermediates (tests/test_backbone_gpu.py: _run_case)
KINDS = ("t1", "ap", "dz2", "g", "s_x", "dap", "dz0")

# (in_ch, block_config, (D, H, W), N): the smallest extents that reach each tile branch (tests/test_backbone_gpu.py: MATRIX, CASES, the
# K-split case)
CASES = {
    "w17": (2, (2, 2), (24, 40, 66), 2),
    "w33": (1, (2, 2), (16, 24, 130), 2),
    "n4_20": (2, (2, 2), (80, 80, 80), 4),
    "tile64": (2, (3, 2), (48, 48, 160), 2),
    "onelayer": (2, (1, 3), (32, 40, 72), 2),
    "narrow": (2, (2, 2, 2), (40, 36, 44), 3),
    "ksplit": (2, (3, 3), (24, 20, 36), 3),
}

# Max-norm relative error, per case and region kind, of torch's own fp32 evaluation of the oracle against the fp64 oracle that takes the
# fp32 run's ReLU branches and pool winners: what plain fp32 arithmetic costs at these extents.  Measured on the CPU
# (tests/test_backbone_backward_taps_cpu.py: test_fp32_floor prints the figures) times 1.5, rounded up (the fp32 sums depend on the
# thread count); every entry must stay <= 1e-5, a tenth of BAR.
FLOOR = {
    "w17": {"t1": 3.7e-6, "ap": 3.6e-6, "dz2": 1.8e-6, "g": 1.4e-6, "s_x": 4.5e-6, "dap": 7.4e-7, "dz0": 1.1e-6},
    "w33": {"t1": 2.3e-6, "ap": 1.7e-6, "dz2": 1.5e-6, "g": 1.1e-6, "s_x": 2.2e-6, "dap": 9.3e-7, "dz0": 7.9e-7},
    "n4_20": {"t1": 3.7e-6, "ap": 3.4e-6, "dz2": 1.3e-6, "g": 1.1e-6, "s_x": 4.5e-6, "dap": 6.0e-7, "dz0": 6.6e-7},
    "tile64": {"t1": 4.3e-6, "ap": 2.3e-6, "dz2": 1.6e-6, "g": 1.1e-6, "s_x": 3.8e-6, "dap": 8.6e-7, "dz0": 9.2e-7},
    "onelayer": {"t1": 5.0e-6, "ap": 2.4e-6, "dz2": 1.4e-6, "g": 1.2e-6, "s_x": 3.7e-6, "dap": 9.5e-7, "dz0": 1.4e-6},
    "narrow": {"t1": 5.6e-6, "ap": 2.4e-6, "dz2": 3.3e-6, "g": 3.8e-6, "s_x": 6.8e-6, "dap": 3.4e-6, "dz0": 3.9e-6},
    "ksplit": {"t1": 3.5e-6, "ap": 3.5e-6, "dz2": 2.1e-6, "g": 1.7e-6, "s_x": 4.6e-6, "dap": 1.8e-6, "dz0": 1.9e-6},
}


def case_inputs(in_ch, blocks, dhw, n):
    cfg = R.DenseNetCfg(in_channels=in_ch, block_config=blocks)
    x = torch.from_numpy(synth.uniform(f"bb/{n}x{in_ch}x{dhw}", (n, in_ch) + tuple(dhw)))
    return cfg, x


def oracle_run(cfg, x, dtype=torch.float64, relu_masks=None, drop_masks=None, pool_taps=None):
    """Training forward and backward (cotangent: the stream "bb/cot", as _run_case) of the oracle in `dtype`.  Returns (sd, taps, h):
    the state dict with every parameter's .grad, the taps with the retained gradients, the output."""
    sch = R.densenet_schema(cfg)
    sd = {k: (v.to(dtype).requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in synth_sd(sch, "densenet.").items()}
    if drop_masks is not None:
        drop_masks = {k: m.to(dtype) for k, m in drop_masks.items()}
    taps = {}
    h = R.densenet_backbone(sd, x.to(dtype), cfg, True, taps=taps, relu_masks=relu_masks, drop_masks=drop_masks, pool_taps=pool_taps)
    cot = torch.from_numpy(synth.uniform("bb/cot", tuple(h.shape))).to(dtype)
    (h * cot).sum().backward()
    return sd, taps, h


def own_branches(taps, x_shape):
    """The ReLU branches and the stem's pool winners that an oracle run took itself, in the form densenet_backbone imposes them."""
    masks = {}
    for k, t in taps.items():
        if k == "norm0":
            masks["relu0"] = (t.detach() > 0).to(torch.uint8)
        elif k.endswith("n1") or k.endswith("n2"):
            masks[k[:-2] + "r" + k[-1]] = (t.detach() > 0).to(torch.uint8)
        elif k.startswith("t") and k.endswith("n"):
            masks[k[:-1]] = (t.detach() > 0).to(torch.uint8)
    t0 = F.relu(taps["norm0"].detach())
    _, idx = F.max_pool3d(t0, kernel_size=3, stride=2, padding=1, return_indices=True)
    d, h, w = t0.shape[2:]
    do, ho, wo = idx.shape[2:]
    ar = lambda m: torch.arange(m, dtype=torch.long)
    kd = idx // (h * w) + 1 - (2 * ar(do))[:, None, None]          # padded coordinate = 2 * window + tap
    kh = (idx // w) % h + 1 - (2 * ar(ho))[None, :, None]
    kw = idx % w + 1 - (2 * ar(wo))[None, None, :]
    return masks, (kd * 9 + kh * 3 + kw).to(torch.uint8)


def batch_stats(x, eps=R.BN_EPS):
    """Per-channel (mean, rstd, xhat) of a batch norm in training: biased variance."""
    dims = (0,) + tuple(range(2, x.dim()))
    mean = x.mean(dims, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dims, keepdim=True) + eps)
    return mean, rstd, (x - mean) * rstd


def bn_backward(G, x, gamma=None):
    """csrc/common.hpp BnBwd: dX = gamma * rstd * (G - mean G - xhat * mean(G * xhat)); `gamma` None when G already carries it."""
    dims = (0,) + tuple(range(2, x.dim()))
    _, rstd, xhat = batch_stats(x)
    dx = rstd * (G - G.mean(dims, keepdim=True) - xhat * (G * xhat).mean(dims, keepdim=True))
    return dx if gamma is None else dx * gamma.view(1, -1, *([1] * (x.dim() - 2)))


def _gamma(sd, key, c):
    return sd[key].detach()[:c].view(1, c, 1, 1, 1)


def build_reference(cfg, sd, taps, relu_masks=None):
    """What every region holds (see the module docstring), from one oracle_run.  `relu_masks`: the imposed branches of the transition
    ReLUs (for `ap`); without them the oracle's own."""
    ref = {}
    nb = len(cfg.block_config)
    ref[("dz0",)] = taps["norm0"].grad
    for b, nl in enumerate(cfg.block_config):
        xb = taps[f"block{b + 1}"].detach()
        G = torch.zeros_like(xb)
        for l in range(nl):
            p = f"backbone.denseblock{b + 1}.denselayer{l + 1}.layers"
            n1 = taps[f"b{b + 1}l{l + 1}n1"]
            c = n1.shape[1]
            G[:, :c] += _gamma(sd, p + ".norm1.weight", c) * n1.grad
            ref[("dz2", b, l)] = taps[f"b{b + 1}l{l + 1}n2"].grad
            ref[("t1", b, l)] = taps[f"b{b + 1}l{l + 1}t1"].detach()
        if b == nb - 1:
            G += _gamma(sd, "backbone.norm5.weight", xb.shape[1]) * taps["norm5"].grad
        else:
            tn = taps[f"t{b + 1}n"]
            G += _gamma(sd, f"backbone.transition{b + 1}.norm.weight", xb.shape[1]) * tn.grad
            w = sd[f"backbone.transition{b + 1}.conv.weight"].detach()
            ref[("dap", b)] = F.conv_transpose3d(taps[f"trans{b + 1}"].grad, w)
            m = (tn.detach() > 0) if relu_masks is None else relu_masks[f"t{b + 1}"]
            ref[("ap", b)] = F.avg_pool3d(tn.detach() * m.to(tn.dtype), kernel_size=2, stride=2)
        ref[("g", b)] = G
        ref[("s_x", b)] = region_sums(G, xb)
    return ref


def region_sums(G, x):
    """(2, C) fp64: S1 = sum G, S2 = sum G * xhat."""
    dims = (0,) + tuple(range(2, x.dim()))
    _, _, xhat = batch_stats(x.double())
    return torch.stack([G.double().sum(dims), (G.double() * xhat).sum(dims)])


def worst(got, ref):
    """(max-norm relative error, index of the worst element): max |got - ref| / max |ref|; the index is (n, c, d, h, w) for a region and
    (row, c) for the sums.  A NaN in `got` is the worst element."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    diff = (got - ref).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    i = int(diff.argmax())
    return float(diff.reshape(-1)[i] / max(float(ref.abs().max()), 1e-30)), tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))


def compare(got, ref):
    """{kind: (worst error, region key, index)} over every region of `ref`; a region missing from `got` is an error."""
    out = {}
    for key, r in ref.items():
        assert key in got, key
        e, idx = worst(got[key], r)
        if key[0] not in out or e > out[key[0]][0]:
            out[key[0]] = (e, key, idx)
    return out


def l2_criterion(got, ref, gl2):
    """err / tol of the parameter-gradient criterion of tests/test_backbone_gpu.py::_run_case: |got - ref| <= 1e-3 |ref| + 1e-5 |g_all|."""
    return float((got.double() - ref.double()).norm()) / (1e-3 * float(ref.norm()) + 1e-5 * gl2)


def grad_l2(sd):
    return float(torch.sqrt(sum((v.grad.double() ** 2).sum() for v in sd.values() if getattr(v, "grad", None) is not None)))
