"""The restated dropout masks (tests/_util.py: drop_scale_ref and the element-wise keyings) and the oracle's mask hooks, on the CPU.
The restatement is read off csrc/common.hpp, so it is pinned from two sides: here (it behaves like a Bernoulli(p) stream whose keys
all matter) and on the device (tests/test_backbone_gpu.py: the mask read off the concat buffer equals it for every (layer, n, c)).

Bounds are derived, not measured: the zero fraction of K independent Bernoulli(p) draws has standard deviation sqrt(p(1-p)/K); two
independent masks agree with probability p^2 + (1-p)^2.  Both are held to 4 * sqrt(p(1-p)/K)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from oracle import synth
from tests import _util as U
from tests._util import synth_sd

LAYERS, NS, CS = 58, 4, 32          # DenseNet121: 58 dense layers x 4 samples x 32 growth channels = 7424 draws
K = LAYERS * NS * CS
SEED = 0x1234_5678_9ABC_DEF0


def _channel_draws(seed, p, layer0=0, n0=0):
    return np.stack([U.drop_scale_ref(seed, layer0 + l, n0 + np.arange(NS)[:, None], np.arange(CS)[None, :], p) for l in range(LAYERS)])


def _bound(p, k=K):
    return 4.0 * np.sqrt(p * (1.0 - p) / k)


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_zero_fraction_and_keep_scale(p):
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    draws = {
        "channel": _channel_draws(SEED, p),
        "channel, seed >= 2^63": _channel_draws(SEED | (1 << 63), p),
        "features": U.feat_drop_mask_ref(SEED, 2, K // 2, p),                      # n*f crosses 1024
        "features past 2^20": U.feat_drop_mask_ref(SEED, 2, 600000, p).reshape(-1)[(1 << 20) - K // 2:(1 << 20) + K // 2],
        "mlp rows": np.stack([U.mlp_row_mask_ref(SEED, l, K // 8, p) for l in range(8)]),
        "resnet elements": U.resnet_elem_mask_ref(SEED, K, p),
    }
    for name, m in draws.items():
        assert m.size == K and m.dtype == np.float32, name
        assert set(np.unique(m).tolist()) == {0.0, float(keep)}, name               # 0 or exactly fl32(1 / (1 - p))
        zf = float((m == 0).mean())
        print(f"p={p} {name}: zero fraction {zf:.4f} (bound {_bound(p):.4f})")
        assert abs(zf - p) < _bound(p), (name, zf)
    if p == 0.5:
        assert float(keep) == 2.0
    else:
        assert abs(float(keep) - 1.25) <= 1.25 * 2.0 ** -23


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_every_key_changes_the_mask(p):
    base = _channel_draws(SEED, p)
    q = p * p + (1.0 - p) * (1.0 - p)
    others = {
        "other layers": _channel_draws(SEED, p, layer0=LAYERS),
        "next layer": _channel_draws(SEED, p, layer0=1),
        "other samples": _channel_draws(SEED, p, n0=NS),
        "next sample": _channel_draws(SEED, p, n0=1),
        "seed + 1": _channel_draws(SEED + 1, p),
        "seed bit 33": _channel_draws(SEED ^ (1 << 33), p),
        "seed bit 47": _channel_draws(SEED ^ (1 << 47), p),
        "seed bit 63": _channel_draws(SEED ^ (1 << 63), p),
    }
    for name, m in others.items():
        assert not np.array_equal(m, base), name
        agree = float((m == base).mean())
        print(f"p={p} {name}: agreement {agree:.4f} (independent: {q:.4f}, bound {_bound(p):.4f})")
        assert abs(agree - q) < _bound(p), (name, agree, q)
    # the element-wise keyings: the mask of one seed against another's, and the MLP's two stacks (first_layer_id 0 / 5)
    for name, a, b in (("features", U.feat_drop_mask_ref(SEED, 4, K // 4, p), U.feat_drop_mask_ref(SEED ^ (1 << 63), 4, K // 4, p)),
                       ("resnet", U.resnet_elem_mask_ref(SEED, K, p), U.resnet_elem_mask_ref(SEED ^ (1 << 40), K, p)),
                       ("mlp layers 0 / 5", U.mlp_row_mask_ref(SEED, 0, K, p), U.mlp_row_mask_ref(SEED, 5, K, p))):
        assert not np.array_equal(a, b), name
        assert abs(float((a == b).mean()) - q) < _bound(p), name


def test_p_zero_is_all_ones():
    assert np.array_equal(_channel_draws(SEED, 0.0), np.ones((LAYERS, NS, CS), np.float32))
    assert np.array_equal(U.feat_drop_mask_ref(SEED, 3, 12, 0.0), np.ones((3, 12), np.float32))
    assert np.array_equal(U.mlp_row_mask_ref(SEED, 2, 7, 0.0), np.ones(7, np.float32))
    assert np.array_equal(U.resnet_elem_mask_ref(SEED, 100, 0.0), np.ones(100, np.float32))


def test_vectorised_form_equals_python_integers():
    """The numpy uint64 form against the same recipe in unbounded Python integers reduced modulo 2^64 (one draw at a time)."""
    M = (1 << 64) - 1

    def one(seed, layer, n, c, p):
        x = (seed + 0x9E3779B97F4A7C15 * (((layer & 0xFFFFFFFF) << 40) ^ ((n & 0xFFFFFFFF) << 20) ^ (c & 0xFFFFFFFF))) & M
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        x ^= x >> 31
        u = np.float32(x >> 40) * np.float32(1.0 / 16777216.0)
        return np.float32(0) if u < np.float32(p) else np.float32(1) / (np.float32(1) - np.float32(p))

    for seed in (0, 1, SEED, (1 << 64) - 1, 1 << 63):
        for layer in (0, 57, 0x7E0005, 0x7F0001):
            got = U.drop_scale_ref(seed, layer, np.arange(3)[:, None], np.array([0, 31, 1023])[None, :], 0.2)
            want = np.array([[one(seed, layer, n, c, 0.2) for c in (0, 31, 1023)] for n in range(3)], np.float32)
            assert np.array_equal(got, want), (seed, layer)


# ---- the oracle's hooks ---------------------------------------------------------------------------------------------------------
def _small():
    cfg = R.DenseNetCfg(in_channels=2, block_config=(2, 2))
    sch = R.densenet_schema(cfg)
    x = torch.from_numpy(synth.uniform("dropcpu/x", (3, 2, 32, 32, 32)))
    return cfg, sch, x


def test_all_ones_masks_reproduce_the_plain_oracle_bitwise():
    cfg, sch, x = _small()
    sd0, sd1 = synth_sd(sch, "densenet."), synth_sd(sch, "densenet.")
    ones = {k: torch.ones_like(v) for k, v in U.backbone_drop_masks(cfg, SEED, 3, 0.2).items()}
    assert len(ones) == 4
    a = R.densenet_forward(sd0, x, cfg, True)
    b = R.densenet_forward(sd1, x, cfg, True, drop_masks={k: v.float() for k, v in ones.items()}, feat_drop_mask=torch.ones(3, cfg.feature_channels))
    assert torch.equal(a, b)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k                                       # running statistics too
    msch = R.mlp_schema(32, 2, 12)
    c = torch.from_numpy(synth.uniform("dropcpu/c", (5, 32)))
    m0, m1 = synth_sd(msch, "mlp."), synth_sd(msch, "mlp.")
    assert torch.equal(R.mlp_features(m0, c, True, 0.0), R.mlp_features(m1, c, True, 0.2, drop_masks=[torch.ones(5)] * 6))
    fsch = R.multimodal_schema(cfg, 32, 2, 12)
    f0, f1 = synth_sd(fsch, "fusion."), synth_sd(fsch, "fusion.")
    o0 = R.multimodal_forward(f0, x, c[:3], cfg, True, True, mlp_dropout=0.0)
    o1 = R.multimodal_forward(f1, x, c[:3], cfg, True, True, mlp_dropout=0.2, drop_masks={k: v.float() for k, v in ones.items()},
                              feat_drop_mask=torch.ones(3, 12), mlp_drop_masks=[torch.ones(3)] * 6)
    assert torch.equal(o0, o1)
    rsch = R.resnet18_schema(2)
    xr = torch.from_numpy(synth.uniform("dropcpu/r", (2, 1, 4, 16, 16)))
    r0, r1 = synth_sd(rsch, "r3d."), synth_sd(rsch, "r3d.")
    taps = {}
    y0 = R.resnet18_forward(r0, xr, True, taps=taps)
    y1 = R.resnet18_forward(r1, xr, True, 0.5, drop_masks={k: torch.ones_like(v) for k, v in taps.items() if k.startswith("layer")})
    assert torch.equal(y0, y1)


def test_imposed_mask_has_dropout3d_semantics():
    """A 0 / 1/(1-p) mask: the dropped (n, c) channels of the layer's slice are zero in the concat tensor, the survivors are the
    undropped values times 1/(1-p) -- what F.dropout3d does with that channel choice."""
    cfg = R.DenseNetCfg(in_channels=2, block_config=(1, 1))
    sch = R.densenet_schema(cfg)
    x = torch.from_numpy(synth.uniform("dropcpu/x3", (3, 2, 32, 32, 32))).double()
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in synth_sd(sch, "densenet.").items()}
    masks = U.backbone_drop_masks(cfg, 7, 3, 0.5)
    m = masks["b1l1"]
    assert float(m.min()) == 0.0 and float(m.max()) == 2.0
    t_drop, t_plain = {}, {}
    R.densenet_backbone(dict(sd), x, cfg, True, taps=t_drop, drop_masks={"b1l1": m})
    R.densenet_backbone(dict(sd), x, cfg, True, taps=t_plain)
    new_d, new_p = t_drop["block1"][:, cfg.init_features:], t_plain["block1"][:, cfg.init_features:]
    assert torch.equal(new_d, new_p * m[:, :, None, None, None])
    assert torch.equal(t_drop["block1"][:, :cfg.init_features], t_plain["block1"][:, :cfg.init_features])
    dead = (new_d.abs().amax(dim=(2, 3, 4)) == 0)
    assert torch.equal(dead, m == 0)
    # torch's own op with the same channel choice: only the random draw differs, so compare through the structure of its output
    torch.manual_seed(0)
    y = F.dropout3d(new_p, 0.5, True)
    ratio = (y.abs().amax(dim=(2, 3, 4)) / new_p.abs().amax(dim=(2, 3, 4)))
    assert set(ratio.flatten().tolist()) <= {0.0, 2.0}


# ---- seeds of the small-batch MLP cases (tests/test_ops_gpu.py) ---------------------------------------------------------------------
def test_mlp_dropout_case_seeds_are_well_conditioned():
    """Batch norm over two to four rows of which some are dropped (constant) rows is ill-conditioned (finding 1): fp32
    and fp64 then disagree by more than any kernel error.  The seeds of the N <= 4 cases are chosen so that torch's own fp32
    evaluation with the restated masks stays inside the comparison's tolerance of the fp64 one; this test keeps that true."""
    from tests._dropout_cases import CASES, fp32_vs_fp64, well_formed
    for case in CASES:
        assert well_formed(case), case                                          # a dropped row; a kept row in every layer
        if case.n <= 4:
            e = fp32_vs_fp64(case)                                              # worst err / tolerance over every compared quantity
            print(case, "fp32 oracle against fp64 oracle: worst err / tolerance", e)
            assert e < 1.0, (case, e)


def test_fusion_step_seed_is_well_conditioned():
    """The same rule for the clinical MLP inside the full-step dropout test (tests/test_fusion_gpu.py, N = 4): its masks, derived from
    torch.manual_seed(FUSION_TORCH_SEED) the way ops.next_seed() derives them, keep torch's fp32 evaluation within the tolerance."""
    from tests._dropout_cases import FUSION_TORCH_SEED, fp32_vs_fp64, fusion_mlp_case, fusion_seeds, well_formed
    seeds = fusion_seeds(FUSION_TORCH_SEED)
    assert len(set(seeds)) == 4 and all(0 <= s < 2 ** 64 for s in seeds) and any(s >= 2 ** 63 for s in seeds)
    case = fusion_mlp_case(FUSION_TORCH_SEED)
    assert well_formed(case)
    e = fp32_vs_fp64(case, "fusion")
    print(case, "fp32 oracle against fp64 oracle: worst err / tolerance", e)
    assert e < 1.0, e


def test_imposed_pool_winners_reproduce_the_plain_oracle_bitwise():
    """`pool_taps` = the oracle's own max-pool winners: output and gradients are those of F.max_pool3d, bit for bit; a window given
    another element shows up in taps["pool_gap"]."""
    cfg, sch, x = _small()
    sd0, sd1 = synth_sd(sch, "densenet.", requires_grad=True), synth_sd(sch, "densenet.", requires_grad=True)
    t0 = {}
    a = R.densenet_backbone(sd0, x, cfg, True, taps=t0)
    relu0 = F.relu(t0["norm0"].detach())
    _, idx = F.max_pool3d(relu0, 3, 2, 1, return_indices=True)
    d, h, w = relu0.shape[2:]
    do, ho, wo = idx.shape[2:]
    ar = torch.arange
    kd = idx // (h * w) - (2 * ar(do)[:, None, None] - 1)
    kh = (idx // w) % h - (2 * ar(ho)[None, :, None] - 1)
    kw = idx % w - (2 * ar(wo)[None, None, :] - 1)
    pool = (kd * 9 + kh * 3 + kw).to(torch.uint8)
    t1 = {}
    b = R.densenet_backbone(sd1, x, cfg, True, taps=t1, pool_taps=pool)
    assert torch.equal(a, b) and float(t1["pool_gap"].abs().max()) == 0.0
    a.square().sum().backward()
    b.square().sum().backward()
    assert torch.equal(sd0["backbone.conv0.weight"].grad, sd1["backbone.conv0.weight"].grad)
    pool[0, 0, 1, 1, 1] = (int(pool[0, 0, 1, 1, 1]) + 1) % 27           # an interior window: every tap is inside the volume
    t2 = {}
    R.densenet_backbone(synth_sd(sch, "densenet."), x, cfg, True, taps=t2, pool_taps=pool)
    assert int((t2["pool_gap"] > 0).sum()) <= 1 and float(t2["pool_gap"].min()) >= 0.0
