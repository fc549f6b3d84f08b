"""White-box parity of the HIP DenseNet backbone (forward intermediates, running statistics, every parameter
gradient) against the CPU oracle on the same synthetic inputs.  fp32; tolerances written per check."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle import synth
from tests._util import backbone_drop_masks, channel_drop_mask, rel_err, synth_sd

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


def _check_device_masks(nb, masks):
    """The channel-dropout decisions read off the device (a layer's new channels in the concat buffer: all-zero or not) against the
    restated masks, for every (layer, n, c); every layer's mask has a dropped and a kept entry, so no layer is covered by luck."""
    alive = nb.device_drop_masks()
    assert set(alive) == set(masks)
    for k, m in masks.items():
        assert bool((m == 0).any()) and bool((m != 0).any()), k
        assert torch.equal(alive[k], m != 0), (k, int((alive[k] != (m != 0)).sum()))


def _run_case(in_ch, blocks, dhw, n, full=True, dropout=0.0, seed=0, options=(), keep=None):
    """Truth = the oracle evaluated in fp64 (the fp32 oracle itself is only within ~3e-5 of it at 64^3, see
    DESIGN.md "Tolerances"); bar = 1e-4 relative (north star) on every intermediate, the output and the running
    statistics; gradients: per-tensor L2 error <= 1e-3*|g| + 1e-5*|g_all| (several gradients are analytically 0).
    `full=False`: extents whose last block has a single voxel per sample -- two-sample batch norm is ill-conditioned
    there (fp32 and fp64 oracles disagree by >10 %), so only the blocks before it are compared.
    `dropout` > 0: the plan drops channels with stream `seed`; the oracle gets the restated masks (tests/_util.py) of every layer
    imposed, as it gets the device's ReLU branches, and the masks are checked against the device's own decisions first."""
    from tests._native import NativeBackbone, backbone_run_keys
    cfg = R.DenseNetCfg(in_channels=in_ch, block_config=blocks)
    sch = R.densenet_schema(cfg)
    x = torch.from_numpy(synth.uniform(f"bb/{n}x{in_ch}x{dhw}", (n, in_ch) + dhw))
    nb = NativeBackbone(cfg, n, *dhw, dropout=dropout)
    for name, value in options:
        nb.set_option(name, value)
    flat, run = nb.flatten(synth_sd(sch, "densenet."))
    xg = x.cuda()
    out = nb.forward(flat, run, xg, training=True, seed=seed)
    torch.cuda.synchronize()
    drop_masks = None
    if dropout > 0:
        drop_masks = backbone_drop_masks(cfg, seed, n, dropout)
        _check_device_masks(nb, drop_masks)
    # fp64 oracle taking the SAME ReLU branches as the device (ReLU'(0) is a convention; near-zero pre-activations would
    # otherwise make any two fp32 implementations disagree by percents in block 4, where a channel has N*V = 16 samples)
    masks = nb.relu_masks(flat) if full else None
    # ... and routing the stem's max-pool gradients to the SAME voxels: which of two elements that agree to fp32 resolution wins a
    # window is a branch decision too.  At 128^3 a handful of the 4.2 M windows are such near-ties; torch's own fp32 evaluation of the
    # oracle (same ReLU branches) then misses the conv0.weight tolerance against the fp64 one exactly as the device does (err/tol 2.003
    # both at p = 0.2, 0.93 at p = 0) while the device's weight-gradient kernel fed the same dz0 is at 0.0006.  That the imposed
    # winners ARE (near-)maxima is asserted below, so a pool kernel that picks a wrong element is still caught.
    pool = nb.pool_taps() if full else None
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v)
          for k, v in synth_sd(sch, "densenet.").items()}
    taps = {}
    h = R.densenet_backbone(sd, x.double(), cfg, True, taps=taps, relu_masks=masks, drop_masks=drop_masks, pool_taps=pool)
    if full:
        gap = taps["pool_gap"]
        print("max-pool windows won by another element than in fp64:", int((gap > 0).sum()), "of", gap.numel(), "largest gap / max",
              float(gap.max() / taps["stem"].detach().abs().max()))
        assert float(gap.max()) <= 1e-4 * float(taps["stem"].detach().abs().max())       # the forward bar: never a materially smaller element
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
    g = nb.backward(flat, xg, cot.cuda(), seed=seed)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(nb=nb, out=out, grad=g, run=run, flat=flat, x=xg, cot=cot.cuda())
    got = nb.unflatten(g.cpu())
    gl2 = float(torch.sqrt(sum((sd[k].grad ** 2).sum() for k in got)))
    worst = (0.0, "")
    bad, ratios = [], []
    for k, v in got.items():
        ref = sd[k].grad
        err = float((v.double() - ref).norm())
        tol = 1e-3 * float(ref.norm()) + 1e-5 * gl2
        worst = max(worst, (err / tol, k))
        ratios.append((err / tol, k))
        if err > tol:
            bad.append((k, err, float(ref.norm()), float(v.double().norm())))
    print("largest gradient err/tol:", sorted(ratios, reverse=True)[:4])
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


# ---- dropout on ------------------------------------------------------------------------------------------------------------------
# The dropout scale of a dense layer's new channels is a pure function of (seed, layer, n, c) that every kernel which needs it computes
# for itself: the conv2 forward epilogues (fp32-MFMA, its K-split variant, bf16x3), the conv2 data-gradient prologue and the bf16 split
# pass, both conv2 weight-gradient kernels (per staged sample), through the batched table and the block-range backward.  With p = 0 it
# returns 1 before it looks at its arguments; these cases run p > 0 with the restated masks imposed on the fp64 oracle, at the p = 0
# tolerances (a 0 / fl32(1/(1-p)) factor does not change conditioning).
SEED_A = 0x9E3779B97F4A7C15        # >= 2^63: what ops.next_seed() produces are full 64-bit values; the binding must pass them unsigned
SEED_B = 20260213


def _drop_case(in_ch, blocks, dhw, n, p, seed, **kw):
    errs, worst = _run_case(in_ch, blocks, dhw, n, dropout=p, seed=seed, **kw)
    print(f"dropout {p} seed {seed:#x}: forward rel errors", errs, "worst gradient (err/tol, name)", worst)
    return errs, worst


@pytest.mark.parametrize("in_ch,blocks,dhw,n", MATRIX)
def test_backbone_dropout_parity_tile_matrix(in_ch, blocks, dhw, n):
    """One extent per tile branch (ragged W = 17 / 33, N = 4, the one-layer block) at p = 0.2."""
    _drop_case(in_ch, blocks, dhw, n, 0.2, SEED_A if n == 2 else SEED_B)


def _wg3_ranges(nb, b, l, n):
    """Tile ranges of the workgroups of dense layer (b, l)'s conv2 weight gradient, from the plan's own split count and the tile rule of
    csrc/wgrad.hip (`wg3_tile`): (tiles per sample, [(begin, end)])."""
    d, h, w = nb.block_dims()[b]
    td, th, tw = (1, 2, 32) if w > 16 else (1, 4, 16) if w > 8 else (2, 4, 8) if w > 4 else (4, 4, 4)
    per_n = -(-d // td) * -(-h // th) * -(-w // tw)
    ns = nb.query("#ns_c2", b, l)
    return per_n, [(n * per_n * s // ns, n * per_n * (s + 1) // ns) for s in range(ns)]


def _crossings(nb, b, l, n):
    per_n, ranges = _wg3_ranges(nb, b, l, n)
    return [(lo, hi) for lo, hi in ranges for k in range(1, n) if lo < k * per_n < hi]


# (in_ch, blocks, extent, blocks whose conv2 weight-gradient ranges must cross a sample boundary at N = 3)
N3_CASES = [
    # block 1 = 20^3, W % 4 == 0: the pipelined kernel (wgrad.hpp `ld_n != st_n`); 600 tiles in 64 ranges: [196, 206) holds 200 and
    # [393, 403) holds 400 -- the coefficients are rescaled mid-range while the next sample's tile is already staged
    (2, (2, 2), (80, 80, 80), (0,)),
    # block 1 = 8x10x18 (40 tiles per sample in 60 ranges), block 2 = 4x5x9 (8 in 12): every boundary is a range boundary -- N = 3 alone
    # does not make a range cross; kept as the narrow matrix extent, the crossing of the narrow kernels is the next case
    (2, (1, 3), (32, 40, 72), ()),
    # block 2 = 5x4x5 (W = 5: the unpipelined kernel, `n != cur_n`): 3 tiles per sample, 9 tiles in 4 ranges: [2, 4) crosses 3;
    # block 3 = 2^3: one range holds all three samples
    (2, (2, 2, 2), (40, 36, 44), (1, 2)),
]


@pytest.mark.parametrize("in_ch,blocks,dhw,cross", N3_CASES)
def test_backbone_dropout_parity_sample_boundaries(in_ch, blocks, dhw, cross):
    """N = 2 / 4 with an even split count put every sample boundary on a range boundary of the weight-gradient kernels, so their
    per-sample refresh of the dropout scale never runs mid-range (true of every matrix case at N = 2).  N = 3 at p = 0.2; that the
    ranges do cross is computed from the plan's own split counts, not assumed."""
    keep = {}
    _drop_case(in_ch, blocks, dhw, 3, 0.2, SEED_B, keep=keep)
    nb = keep["nb"]
    for b in range(len(blocks)):
        got = [_crossings(nb, b, l, 3) for l in range(blocks[b])]
        print("block", b + 1, "ranges that cross a sample boundary:", got[0])
        assert all(bool(g) == (b in cross) for g in got), (b, got)


def test_backbone_dropout_parity_64():
    _drop_case(2, (6, 12, 24, 16), (64, 64, 64), 2, 0.2, SEED_A)


def test_backbone_dropout_parity_bench_configuration_128():
    """What bench.py times: 2 x 2 x 128^3, dropout 0.2 -- every intermediate, the running statistics and all 364 gradients."""
    _drop_case(2, (6, 12, 24, 16), (128, 128, 128), 2, 0.2, SEED_B)


def _harsh_seed(blocks, n, p, growth=32):
    """First seed (CPU, restated mask) whose masks have, in one layer, a channel dropped in every sample -- the next norm1 then sees a
    channel of zero variance -- and a channel kept in every sample."""
    for seed in range(1, 1000):
        for layer in range(sum(blocks)):
            m = channel_drop_mask(seed, layer, n, growth, p)
            if bool((m == 0).all(axis=0).any()) and bool((m != 0).all(axis=0).any()):
                return seed, layer
    raise AssertionError("no such seed")


def test_backbone_dropout_parity_half_dropped_with_dead_channel():
    blocks, n, p = (3, 2), 3, 0.5
    seed, layer = _harsh_seed(blocks, n, p)
    m = channel_drop_mask(seed, layer, n, 32, p)
    assert bool((m == 0).all(axis=0).any()) and bool((m != 0).all(axis=0).any())        # the coverage is not luck
    print("seed", seed, "layer", layer, "channels dropped in all samples", np.nonzero((m == 0).all(axis=0))[0].tolist())
    _drop_case(2, blocks, (32, 40, 72), n, p, seed)


def test_backbone_dropout_parity_with_and_without_k_split():
    """The K-split forward of the small extents has an epilogue of its own.  One small-extent plan with the split (default) and
    without (option "no_kz"): both against the fp64 oracle, and against each other at the tolerances of tests/test_kz_handoff_gpu.py."""
    a, b = {}, {}
    _drop_case(2, (3, 3), (24, 20, 36), 3, 0.2, SEED_A, keep=a)
    _drop_case(2, (3, 3), (24, 20, 36), 3, 0.2, SEED_A, keep=b, options=(("no_kz", 1),))
    eo = float((a["out"] - b["out"]).abs().max() / b["out"].abs().max())
    eg = float((a["grad"] - b["grad"]).norm() / b["grad"].norm())
    print("split against unsplit: output", eo, "gradient", eg)
    assert eo < 2e-4 and eg < 3e-2, (eo, eg)


def _small_plan(dropout):
    from tests._native import NativeBackbone
    cfg = R.DenseNetCfg(in_channels=2, block_config=(2, 2, 2))
    n, dhw = 3, (40, 36, 44)
    nb = NativeBackbone(cfg, n, *dhw, dropout=dropout)
    flat, run = nb.flatten(synth_sd(R.densenet_schema(cfg), "densenet."))
    x = torch.from_numpy(synth.uniform("bb/drop/small", (n, 2) + dhw)).cuda()
    cot = torch.from_numpy(synth.uniform("bb/drop/cot", nb.out_shape)).cuda()
    return cfg, nb, flat, run, x, cot


def test_backbone_dropout_block_range_backward_is_bit_identical():
    """The data-parallel schedule walks the backward in block ranges and recomputes the running layer id from the range's top block:
    any walk must reproduce the single call bit for bit."""
    cfg, nb, flat, run, x, cot = _small_plan(0.2)
    nb.forward(flat, run, x, training=True, seed=SEED_A)
    ref = nb.backward(flat, x, cot, seed=SEED_A).clone()
    assert float(ref.abs().max()) > 0
    for walk in (((2, 2), (1, 1), (0, 0)), ((2, 1), (0, 0))):
        g = torch.zeros_like(ref)
        for hi, lo in walk:
            nb.backward_range(flat, x, cot, hi, lo, seed=SEED_A, grad=g)
        torch.cuda.synchronize()
        assert torch.equal(g, ref), (walk, float((g - ref).abs().max()))


def test_backbone_dropout_repeatability_seeds_and_accumulate():
    cfg, nb, flat, run, x, cot = _small_plan(0.2)
    res = []
    for seed in (SEED_A, SEED_A, SEED_B):
        r = run.clone()
        out = nb.forward(flat, r, x, training=True, seed=seed).clone()
        alive = nb.device_drop_masks()
        g = nb.backward(flat, x, cot, seed=seed).clone()
        torch.cuda.synchronize()
        res.append((out, g, r, alive))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert torch.equal(a, b)                                   # same seed: outputs, gradients, running statistics bit-identical
    assert all(torch.equal(res[0][3][k], res[1][3][k]) for k in res[0][3])
    assert any(not torch.equal(res[0][3][k], res[2][3][k]) for k in res[0][3])      # another seed: another mask ...
    assert not torch.equal(res[0][0], res[2][0])                                   # ... and another output
    nb.forward(flat, run.clone(), x, training=True, seed=SEED_A)
    g1 = nb.backward(flat, x, cot, seed=SEED_A).clone()
    g2 = nb.backward(flat, x, cot, accumulate=True, seed=SEED_A, grad=g1.clone())
    torch.cuda.synchronize()
    assert torch.equal(g1, res[0][1])
    assert rel_err(g2.cpu().numpy(), (2 * g1).cpu().numpy()) < 1e-6


def test_backbone_dropout_plan_in_eval_mode_is_the_plain_plan():
    cfg, nb, flat, run, x, cot = _small_plan(0.2)
    _, nb0, flat0, run0, _, _ = _small_plan(0.0)
    before = run.clone()
    out = nb.forward(flat, run, x, training=False, seed=SEED_A)
    out0 = nb0.forward(flat0, run0, x, training=False, seed=SEED_A)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, out0)
    assert torch.equal(run, before)


@pytest.mark.parametrize("mode", ["0"])
def test_bf16x3_switch_positions_keep_parity(mode):
    """The suite runs with the default kernel selection (conv2 forward / data gradient of extents wider than 16 voxels on three-piece bf16
    MFMAs, csrc/conv3_bf16x3.hip).  The switch is read once per process, so the other position runs in a fresh one: MMNN_BF16X3=0 (the
    fp32-MFMA kernels for every extent) must pass the same tile-matrix parity (ragged W = 17 / 33 included) against the fp64 oracle at the
    same tolerances -- without dropout and with it (test_backbone_dropout_parity_tile_matrix: the fp32-MFMA epilogue and data-gradient
    prologue compute the dropout scale in code of their own)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMNN_BF16X3=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "tile_matrix"], env=env, cwd=root,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"{2 * len(MATRIX)} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
