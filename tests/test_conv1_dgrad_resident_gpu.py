"""The resident-operand conv1 data gradient (csrc/conv1_dgrad.hip) at small shapes: row steps with a ragged last step, a voxel tile that
is partly out of range, the row-group split of the grid, the shapes that must take fprop_kernel instead, and the chain around it with
dropout on.  Every region of the backward against the fp64 oracle with the device's ReLU branches imposed (tests/_backward_taps.py), the
plan's "#conv1_dgrad_resident" counter against the eligibility rule restated here, two identical calls bit for bit, the block-by-block
walk against the single call bit for bit -- and the same with the kernel switched off (plan option "conv1_dgrad_resident" = 0), the
`g` and `s_x` errors of both kernels side by side: the new kernel's may exceed the old one's by the case's fp32 floor at the most.
The kernel takes its fp32 sums in the order of the fprop_kernel tile that the shape would run on, so the parameter gradient and the `g`
regions of options 2 and 0 are also compared bit for bit.

Plan option values: 0 never, 1 (default) only where the kernel measured faster (512 <= V voxels per sample in at most 512 voxel tiles of
64: of the cases here only block 1 of `mloop`), 2 wherever the kernel can run -- the value these cases run the new kernel with; the
counter is checked against the rule under all three."""
import dataclasses

import pytest
import torch

from tests import _backward_taps as T
from tests._util import backbone_drop_masks, synth_sd
from oracle import restatement as R
from oracle import synth

pytestmark = pytest.mark.gpu

SEED_A = 0x9E3779B97F4A7C15        # tests/test_backbone_gpu.py

# (in_ch, block_config, (D, H, W), N, widths); block-1 extents are the input extents / 4
CASES = {
    # block 1: 8 x 8 x 16 voxels, cin 64 .. 192 = 1 .. 3 row steps of 64; block 2: 4 x 4 x 8, cin 112, 144 (no multiple of 64)
    "mloop": (2, (5, 2), (32, 32, 64), 2, None),
    # 6 x 6 x 10 = 360 voxels: a multiple of 4 and of no voxel tile, the last tile is partly out of range
    "vtail": (2, (4,), (24, 24, 40), 2, None),
    # 5 x 6 x 9 = 270 voxels, V % 4 = 2: never eligible
    "odd_v": (2, (3,), (20, 24, 36), 3, None),
    # bottleneck width 64: never eligible (the resident tile is built for 128 operand channels)
    "narrow_k": (2, (3,), (16, 16, 32), 2, {"growth_rate": 16, "init_features": 32}),
    # 4 x 4 x 4 = 64 voxels per sample, cin up to 288: two voxel tiles, the row steps are dealt to row groups
    "rowgroups": (2, (8,), (16, 16, 16), 2, None),
    # 3 samples of 8 x 8 x 16 voxels, cin up to 224: at cin = 224 fprop_kernel runs its 64-voxel tile (two wave groups split K) and the
    # resident kernel follows that order of the sums, at the narrower layers the order of the 32-voxel tile (eight wave groups)
    "ksplit2": (2, (6,), (32, 32, 64), 3, None),
}

# fp32 floor of `g` and `s_x` per case: tests/test_backbone_backward_taps_cpu.py::measure_floor's mechanism (measure_floor below, on the
# CPU) times 1.5, rounded up; every entry must stay <= 1e-5.
FLOOR = {
    "mloop": {"g": 1.3e-6, "s_x": 3.7e-6},          # measured 8.65e-7 / 2.42e-6 (the dropout run of this case uses the same floor)
    "vtail": {"g": 9.7e-7, "s_x": 2.6e-6},          # 6.45e-7 / 1.71e-6
    "odd_v": {"g": 8.6e-7, "s_x": 2.3e-6},          # 5.71e-7 / 1.47e-6
    "narrow_k": {"g": 1.2e-6, "s_x": 1.8e-6},       # 7.35e-7 / 1.16e-6
    "rowgroups": {"g": 2.1e-6, "s_x": 4.6e-6},      # 1.34e-6 / 3.01e-6
    "ksplit2": {"g": 1.2e-6, "s_x": 3.1e-6},        # 7.83e-7 / 2.03e-6
}


def case_inputs(name):
    in_ch, blocks, dhw, n, widths = CASES[name]
    cfg, x = T.case_inputs(in_ch, blocks, dhw, n)
    if widths:
        cfg = dataclasses.replace(cfg, **widths)
    return cfg, x, dhw, n


def measure_floor(name):
    """{kind: error} of torch's fp32 evaluation of the oracle against the fp64 oracle with the fp32 run's branches imposed."""
    cfg, x, _, _ = case_inputs(name)
    sd32, taps32, _ = T.oracle_run(cfg, x, dtype=torch.float32)
    masks, winners = T.own_branches(taps32, x.shape)
    sd64, taps64, _ = T.oracle_run(cfg, x, relu_masks=masks, pool_taps=winners)
    assert float(taps64["pool_gap"].max()) <= 1e-4 * float(taps64["stem"].detach().abs().max())
    res = T.compare(T.build_reference(cfg, sd32, taps32, masks), T.build_reference(cfg, sd64, taps64, masks))
    return {k: v[0] for k, v in res.items()}


def expected_count(cfg, nb, n, mode):
    """The eligibility rule of csrc/conv1_dgrad.hip (conv1_dgrad_resident_shape_ok) per dense block: layers that take the new kernel."""
    out, c = [], cfg.init_features
    mid = cfg.bn_size * cfg.growth_rate
    for nl, dims in zip(cfg.block_config, nb.block_dims()):
        v = dims[0] * dims[1] * dims[2]
        cnt = 0
        for l in range(nl):
            cin = c + l * cfg.growth_rate
            ok = mode != 0 and mid == 128 and v % 4 == 0 and cin % 4 == 0 and (cin + 128) * v < 2 ** 31
            if mode == 1:
                ok = ok and v >= 512 and n * -(-v // 64) <= 512
            cnt += int(ok)
        out.append(cnt)
        c = (c + nl * cfg.growth_rate) // 2
    return out


def _backward_checks(nb, cfg, flat, xg, cot, ref, seed, tag):
    """One option setting: walk against the oracle, walk == single call, two single calls bit for bit.  Returns {kind: error}."""
    grad, snap = nb.backward_walk(flat, xg, cot, seed=seed)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in nb.forward_taps().items()}
    got.update({k: v.cpu() for k, v in snap.items()})
    assert set(got) == set(ref), set(got) ^ set(ref)
    res = T.compare(got, ref)
    present = [k for k in T.KINDS if k in res]          # a one-block case has no transition: no "ap" / "dap"
    for kind in present:
        e, key, idx = res[kind]
        print(f"{tag}: {kind:4s} device {e:.2e} worst {key} at {idx}")
    for kind in present:
        e, key, idx = res[kind]
        assert e <= T.BAR, (tag, kind, e, key, idx)
    n, ctot, dims = nb.out_shape[0], nb.block_channels(), nb.block_dims()
    runs = []
    for _ in range(2):
        single = nb.backward(flat, xg, cot, seed=seed)
        torch.cuda.synchronize()
        runs.append((single, [nb.region("g", (n, ctot[b], *dims[b]), b).clone() for b in range(len(dims))]))
    assert torch.equal(grad, runs[0][0]), (tag, float((grad - runs[0][0]).abs().max()))
    assert torch.equal(runs[0][0], runs[1][0]), tag
    for ga, gb in zip(runs[0][1], runs[1][1]):
        assert torch.equal(ga, gb), tag
    return {k: res[k][0] for k in present}, runs[0]


def _run(name, dropout=0.0, seed=0):
    from tests._native import NativeBackbone
    cfg, x, dhw, n = case_inputs(name)
    nb = NativeBackbone(cfg, n, *dhw, dropout=dropout)
    assert nb.query("#conv1_dgrad_resident", 0) == expected_count(cfg, nb, n, 1)[0]      # the default is option 1
    flat, run = nb.flatten(synth_sd(R.densenet_schema(cfg), "densenet."))
    xg = x.cuda()
    out = nb.forward(flat, run, xg, training=True, seed=seed)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    drop = None
    if dropout > 0:
        drop = backbone_drop_masks(cfg, seed, n, dropout)
        alive = nb.device_drop_masks()
        for k, m in drop.items():
            assert torch.equal(alive[k], m != 0), k
    masks, pool = nb.relu_masks(flat), nb.pool_taps()
    sd, taps, h = T.oracle_run(cfg, x, relu_masks=masks, drop_masks=drop, pool_taps=pool)
    assert float(taps["pool_gap"].max()) <= 1e-4 * float(taps["stem"].detach().abs().max())
    ref = T.build_reference(cfg, sd, taps, masks)
    cot = torch.from_numpy(synth.uniform("bb/cot", tuple(h.shape))).cuda()
    tag = name + (f" p={dropout}" if dropout else "")
    err, single = {}, {}
    for mode in (2, 1, 0):
        nb.set_option("conv1_dgrad_resident", mode)
        want = expected_count(cfg, nb, n, mode)
        have = [nb.query("#conv1_dgrad_resident", b) for b in range(len(cfg.block_config))]
        print(f"{tag}: option {mode}: layers on the resident kernel per block {have}, rule {want}")
        assert have == want, (tag, mode, have, want)
        err[mode], single[mode] = _backward_checks(nb, cfg, flat, xg, cot, ref, seed, f"{tag} option={mode}")
    for kind in ("g", "s_x"):
        print(f"{tag}: {kind:4s} resident {err[2][kind]:.2e}  fprop_kernel {err[0][kind]:.2e}  (fp32 floor {FLOOR[name][kind]:.1e})")
    for kind in ("g", "s_x"):
        assert FLOOR[name][kind] <= 1e-5, (name, kind)
        assert err[2][kind] <= err[0][kind] + FLOOR[name][kind], (tag, kind, err[2][kind], err[0][kind])
    # The kernel takes its sums in the order of the fprop_kernel tile that the shape would run on (the in-block K-split of the 64- and
    # 32-voxel tiles, the voxel butterfly of the per-row sums): same fp32 operations in the same order, so the same bits.  (The 128-voxel
    # tile, which none of these cases reaches, adds its two 32-voxel columns before the butterfly: its per-row sums are not reproduced.)
    assert torch.equal(single[2][0], single[0][0]), (tag, float((single[2][0] - single[0][0]).abs().max()))
    for b, (ga, gb) in enumerate(zip(single[2][1], single[0][1])):
        assert torch.equal(ga, gb), (tag, b, float((ga - gb).abs().max()))
    return expected_count(cfg, nb, n, 2)


def test_row_steps_with_a_ragged_last_step():
    assert _run("mloop") == [5, 2]


def test_voxel_tile_partly_out_of_range():
    assert _run("vtail") == [4]


def test_odd_voxel_count_takes_the_fallback():
    assert _run("odd_v") == [0]


def test_narrow_bottleneck_takes_the_fallback():
    assert _run("narrow_k") == [0]


def test_row_groups():
    assert _run("rowgroups") == [8]


def test_both_k_split_orders():
    assert _run("ksplit2") == [6]


def test_row_steps_with_dropout():
    assert _run("mloop", dropout=0.2, seed=SEED_A) == [5, 2]
