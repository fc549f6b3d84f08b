"""The reference of the backward taps (tests/_backward_taps.py) checked on the CPU: it reproduces autograd where autograd can be
asked, plain fp32 stays a decade below the bar, and the comparator sees the planted errors that the parameter-gradient criterion passes."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv3d_weight

from tests import _backward_taps as T
from tests._util import backbone_drop_masks

SEED_B = 20260213         # tests/test_backbone_gpu.py
EXACT = 1e-12


@functools.lru_cache(maxsize=None)
def _oracle(name, dropout=0.0):
    """One fp64 oracle run per (case, dropout) for every test of this module; nobody writes to what it returns."""
    in_ch, blocks, dhw, n = T.CASES[name]
    cfg, x = T.case_inputs(in_ch, blocks, dhw, n)
    drop = backbone_drop_masks(cfg, SEED_B, n, dropout) if dropout > 0 else None
    sd, taps, _ = T.oracle_run(cfg, x, drop_masks=drop)
    return cfg, sd, taps, drop, T.build_reference(cfg, sd, taps)


def _layer(b, l):
    return f"backbone.denseblock{b + 1}.denselayer{l + 1}.layers"


RIGHT = [("w17", 0.0), ("narrow", 0.2)]


@pytest.mark.parametrize("name,dropout", RIGHT)
def test_reference_g_reproduces_conv2_output_gradients(name, dropout):
    """BN-backward (csrc/common.hpp BnBwd, gamma folded into G) of the reference g[b] on a layer's own channels, times the dropout mask,
    is autograd's gradient of that layer's conv2 output; on a block's first channels it is the gradient of the transition output."""
    cfg, sd, taps, drop, ref = _oracle(name, dropout)
    for b, nl in enumerate(cfg.block_config):
        dx = T.bn_backward(ref[("g", b)], taps[f"block{b + 1}"].detach())
        c = dx.shape[1] - nl * cfg.growth_rate
        if b > 0:
            e, idx = T.worst(dx[:, :c], taps[f"trans{b}"].grad)
            assert e < EXACT, (b, e, idx)
        for l in range(nl):
            d = dx[:, c:c + cfg.growth_rate]
            if drop is not None:
                m = drop[f"b{b + 1}l{l + 1}"]
                assert bool((m == 0).any()) and bool((m != 0).any())
                d = d * m.view(*m.shape, 1, 1, 1)
            e, idx = T.worst(d, taps[f"b{b + 1}l{l + 1}y"].grad)
            assert e < EXACT, (b, l, e, idx)
            c += cfg.growth_rate


@pytest.mark.parametrize("name,dropout", RIGHT)
def test_reference_dz2_dap_ap_reproduce_weight_gradients(name, dropout):
    """dz2 feeds the conv1 weight gradient (BN-backward of T1 with gamma2, against ReLU(norm1 output)); dap, un-pooled and masked, is the
    gradient of the transition norm's output, hence that norm's weight and bias gradients; ap is the input of the transition
    convolution's weight gradient.  Each against autograd's."""
    cfg, sd, taps, drop, ref = _oracle(name, dropout)
    for b, nl in enumerate(cfg.block_config):
        for l in range(nl):
            p = _layer(b, l)
            dt1 = T.bn_backward(ref[("dz2", b, l)], ref[("t1", b, l)], sd[p + ".norm2.weight"].detach())
            w = sd[p + ".conv1.weight"]
            e, idx = T.worst(conv3d_weight(F.relu(taps[f"b{b + 1}l{l + 1}n1"].detach()), w.shape, dt1), w.grad)
            assert e < EXACT, ("dz2", b, l, e, idx)
        if b == len(cfg.block_config) - 1:
            continue
        p = f"backbone.transition{b + 1}"
        tn = taps[f"t{b + 1}n"]
        up = ref[("dap", b)].repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4) / 8
        dtn = F.pad(up, [0, tn.shape[4] - up.shape[4], 0, tn.shape[3] - up.shape[3], 0, tn.shape[2] - up.shape[2]]) * (tn.detach() > 0)
        e, idx = T.worst(dtn, tn.grad)
        assert e < EXACT, ("dap", b, e, idx)
        _, _, xhat = T.batch_stats(taps[f"block{b + 1}"].detach())
        assert T.worst((dtn * xhat).sum((0, 2, 3, 4)), sd[p + ".norm.weight"].grad)[0] < EXACT
        assert T.worst(dtn.sum((0, 2, 3, 4)), sd[p + ".norm.bias"].grad)[0] < EXACT
        w = sd[p + ".conv.weight"]
        e, idx = T.worst(conv3d_weight(ref[("ap", b)], w.shape, taps[f"trans{b + 1}"].grad), w.grad)
        assert e < EXACT, ("ap", b, e, idx)


def test_reference_dz0_feeds_the_conv0_weight_gradient():
    cfg, sd, taps, drop, ref = _oracle("w17")
    dy = T.bn_backward(ref[("dz0",)], taps["conv0"].detach(), sd["backbone.norm0.weight"].detach())
    in_ch, blocks, dhw, n = T.CASES["w17"]
    _, x = T.case_inputs(in_ch, blocks, dhw, n)
    w = sd["backbone.conv0.weight"]
    e, idx = T.worst(conv3d_weight(x.double(), w.shape, dy, stride=2, padding=3), w.grad)
    assert e < EXACT, (e, idx)


def measure_floor(name):
    """{kind: error} of torch's fp32 evaluation of the oracle against the fp64 oracle with the fp32 run's branches imposed."""
    in_ch, blocks, dhw, n = T.CASES[name]
    cfg, x = T.case_inputs(in_ch, blocks, dhw, n)
    sd32, taps32, _ = T.oracle_run(cfg, x, dtype=torch.float32)
    masks, winners = T.own_branches(taps32, x.shape)
    sd64, taps64, _ = T.oracle_run(cfg, x, relu_masks=masks, pool_taps=winners)
    assert float(taps64["pool_gap"].max()) <= 1e-4 * float(taps64["stem"].detach().abs().max())
    res = T.compare(T.build_reference(cfg, sd32, taps32, masks), T.build_reference(cfg, sd64, taps64, masks))
    return {k: v[0] for k, v in res.items()}


@pytest.mark.parametrize("name", list(T.CASES))
def test_fp32_floor(name):
    got = measure_floor(name)
    print(name, {k: float(f"{v:.2e}") for k, v in got.items()}, "table", T.FLOOR[name])
    assert set(got) == set(T.KINDS) == set(T.FLOOR[name])
    for k, v in got.items():
        assert T.FLOOR[name][k] <= 1e-5, (name, k)
        assert v <= T.FLOOR[name][k], (name, k, v)


# ---- planted errors: what a tile or halo bug leaves behind -----------------------------------------------------------------------
def _names_voxel(idx, n, d, h, w):
    return (idx[0],) + tuple(idx[2:]) == (n, d, h, w)


def test_planted_lost_tap_in_dz2_is_seen_by_the_comparator_only():
    """One of the 27 taps of the conv2 data gradient lost at one boundary voxel (every channel of one sample): the comparator is two
    decades above the bar and names the voxel; the conv1 weight gradient recomputed from the corrupted dz2 passes the per-tensor L2
    criterion of _run_case (err/tol 0.52).  The criterion is not blind to every lost tap at this extent (N V = 2040): over corner, edge,
    face and interior voxels of block 1 and the taps (1,1,1), (1,1,2), (2,1,2) it gave err/tol 0.07 .. 5.5 for column errors of
    1 .. 70 %, passing 6 of 24; it falls with sqrt(N V), so at 16^3 and 32^3 most of them pass.  The comparator saw every one at 33 .. 1600 x
    the bar."""
    cfg, sd, taps, drop, ref = _oracle("w17")
    b, l, n = 0, 0, 1
    p = _layer(b, l)
    good = ref[("dz2", b, l)]
    D, H, W = good.shape[2:]
    d, h, w = 0, H - 1, W - 1                                       # corner of the ragged W = 17 remainder
    kd, kh, kw = 1, 1, 1                                            # the centre tap
    dy = taps[f"b{b + 1}l{l + 1}y"].grad                            # dt[m, v] = sum_k sum_co W[co, m, k] dY[co, v - k + 1]
    lost = sd[p + ".conv2.weight"].detach()[:, :, kd, kh, kw].t() @ dy[n, :, d - kd + 1, h - kh + 1, w - kw + 1]
    bad = good.clone()
    bad[n, :, d, h, w] -= lost * (taps[f"b{b + 1}l{l + 1}n2"].detach()[n, :, d, h, w] > 0)
    e, idx = T.worst(bad, good)
    print("lost tap: comparator", e, idx)
    assert e > 100 * T.BAR and _names_voxel(idx, n, d, h, w), (e, idx)
    wgt = sd[p + ".conv1.weight"]
    relu1 = F.relu(taps[f"b{b + 1}l{l + 1}n1"].detach())
    g2 = sd[p + ".norm2.weight"].detach()
    ratio = T.l2_criterion(conv3d_weight(relu1, wgt.shape, T.bn_backward(bad, ref[("t1", b, l)], g2)), wgt.grad, T.grad_l2(sd))
    print("lost tap: conv1.weight err/tol", ratio)
    assert ratio < 1.0, ratio


def test_planted_scaled_column_of_g_is_seen_by_the_comparator_only():
    """One voxel column of g (every channel of one sample at one corner voxel) scaled by 0.9: the comparator names it, the conv2 weight
    gradients of the block recomputed from the corrupted g pass the L2 criterion."""
    cfg, sd, taps, drop, ref = _oracle("w17")
    b, n = 0, 1
    good = ref[("g", b)]
    D, H, W = good.shape[2:]
    d, h, w = D - 1, H - 1, W - 1
    bad = good.clone()
    bad[n, :, d, h, w] *= 0.9
    e, idx = T.worst(bad, good)
    print("scaled column: comparator", e, idx)
    assert e > 10 * T.BAR and _names_voxel(idx, n, d, h, w), (e, idx)
    dx = T.bn_backward(bad, taps[f"block{b + 1}"].detach())
    c = dx.shape[1] - cfg.block_config[b] * cfg.growth_rate
    gl2 = T.grad_l2(sd)
    for l in range(cfg.block_config[b]):
        wgt = sd[_layer(b, l) + ".conv2.weight"]
        relu2 = F.relu(taps[f"b{b + 1}l{l + 1}n2"].detach())
        ratio = T.l2_criterion(conv3d_weight(relu2, wgt.shape, dx[:, c:c + cfg.growth_rate], padding=1), wgt.grad, gl2)
        print("scaled column: layer", l, "conv2.weight err/tol", ratio)
        # (layer 1's only consumer is the transition, whose 2x2x2 pool does not reach the odd column w = 16: its G is zero there)
        assert (0.01 if l == 0 else 0.0) < ratio < 1.0, (l, ratio)
        c += cfg.growth_rate
