"""r3d_18 (reference models/resnet.py:5-227) on the HIP kernels: golden vectors from the reference's own class,
every gradient against the fp64 oracle, eval mode, dropout semantics, checkpoint compatibility."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle import synth
from tests._util import load_golden, rel_err, synth_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(dropout=0.0):
    from mmnn_sts_amd.models.resnet import r3d_18
    m = r3d_18(2)
    m.load_state_dict(synth_sd(R.resnet18_schema(2), "r3d."), strict=True)
    m.dropout.p = dropout
    return m.to(DEV)


@pytest.mark.parametrize("tag,shape", [("a", (2, 1, 16, 64, 64)), ("b", (3, 1, 9, 40, 52))])
def test_r3d18_train_step_golden_and_fp64(tag, shape):
    g = load_golden("g10_r3d18.npz")
    m = _model().train()
    x = torch.from_numpy(synth.uniform(f"r3d/x/{tag}", shape))
    y = m(x.to(DEV))
    cot = torch.from_numpy(synth.uniform(f"r3d/cot/{tag}", tuple(y.shape)))
    (y * cot.to(DEV)).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), g[f"{tag}/out"]) < 1e-4                  # north-star bar on the outputs
    sd_dev = m.state_dict()
    for k, v in zip(g[f"{tag}/running_names"], g[f"{tag}/running_chk"]):
        t = sd_dev[str(k)].double()
        np.testing.assert_allclose([t.sum().item(), t.abs().sum().item()], v, rtol=1e-4, atol=1e-6)
    assert int(sd_dev["stem.1.num_batches_tracked"]) == 1 and int(sd_dev["layer4.1.conv2.1.num_batches_tracked"]) == 1
    # every gradient against the oracle evaluated in fp64
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in synth_sd(R.resnet18_schema(2), "r3d.").items()}
    y64 = R.resnet18_forward(sd, x.double(), True)
    (y64 * cot.double()).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), y64.detach().numpy()) < 1e-4
    gl2 = float(torch.sqrt(sum((v.grad ** 2).sum() for v in sd.values() if v.is_floating_point() and v.grad is not None)))
    bad = []
    for k, p in m.named_parameters():
        ref = sd[k].grad
        err = float((p.grad.double().cpu() - ref).norm())
        if err > 2e-3 * float(ref.norm()) + 2e-5 * gl2:
            bad.append((k, err, float(ref.norm())))
    assert not bad, (len(bad), gl2, bad[:6])
    assert len(list(m.named_parameters())) == 65
    # gradients of a few tensors also against the reference's own fp32 numbers (loosely: ReLU branch flips)
    for k in ("fc.weight", "fc.bias"):
        np.testing.assert_allclose(dict(m.named_parameters())[k].grad.cpu().numpy(), g[f"{tag}/grad/{k}"], rtol=2e-3, atol=1e-6)
    m.eval()
    with torch.no_grad():
        assert rel_err(m(x.to(DEV)).cpu().numpy(), g[f"{tag}/eval_out"]) < 1e-4


def test_r3d18_dropout_and_errors():
    m = _model(dropout=0.5).train()
    x = torch.randn(2, 1, 8, 32, 32, device=DEV)
    y1, y2 = m(x), m(x)
    assert torch.isfinite(y1).all() and not torch.equal(y1, y2)                          # fresh element-wise masks per call
    y1.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x), m(x))                                                   # dropout is off in eval mode
    with pytest.raises(ValueError):
        m(torch.randn(2, 2, 8, 32, 32, device=DEV))
    with pytest.raises(RuntimeError):
        m(torch.randn(2, 1, 8, 32, 32))


def test_direct_conv_matches_torch_reference():
    """The generic direct convolution (forward, data gradient, weight gradient) against torch's CPU conv3d in fp64 for the
    kernel / stride / padding combinations r3d_18 uses and a few irregular ones."""
    from mmnn_sts_amd import ops
    cases = [((2, 1, 5, 20, 22), 64, (1, 7, 7), (1, 2, 2), (1, 3, 3)), ((2, 64, 6, 9, 10), 8, (3, 3, 3), 1, 1),
             ((1, 8, 7, 11, 9), 16, (3, 3, 3), 2, 1), ((2, 8, 7, 11, 9), 16, (1, 1, 1), 2, 0), ((3, 5, 4, 6, 7), 19, (2, 3, 1), (1, 2, 3), (1, 0, 2)),
             ((2, 19, 4, 6, 7), 5, (3, 3, 3), 1, 1),              # 19 input channels: a remainder in the data gradient's groups of 16; 5 outputs in a group of 8
             ((2, 3, 5, 8, 9), 4, (1, 2, 2), (2, 3, 3), 0),       # stride beyond the kernel extent: input voxels that no output reads
             ((1, 2, 4, 5, 6), 3, (3, 2, 3), 1, (1, 2, 0)),       # padding >= kernel extent along H: output rows that see padding only
             ((2, 4, 1, 7, 8), 6, (3, 3, 3), 1, 1),               # D = 1 under a 3-tap kernel with padding 1
             ((1, 3, 1, 1, 5), 4, (1, 1, 3), 1, 0)]               # 3 output voxels in all: fewer than the weight gradient's split count
    untouched = 0
    for xs, co, k, s, p in cases:
        x = torch.from_numpy(synth.uniform(f"conv/x/{xs}", xs)).double().requires_grad_(True)
        w = torch.from_numpy(synth.uniform(f"conv/w/{xs}", (co, xs[1]) + tuple(k), 0.3)).double().requires_grad_(True)
        y = torch.nn.functional.conv3d(x, w, None, stride=s, padding=p)
        cot = torch.from_numpy(synth.uniform(f"conv/c/{xs}", tuple(y.shape))).double()
        (y * cot).sum().backward()
        xg = x.detach().float().to(DEV).requires_grad_(True)
        wg = w.detach().float().to(DEV).requires_grad_(True)
        yg = ops.Conv3dDirect.apply(xg, wg, s, p)
        (yg * cot.float().to(DEV)).sum().backward()
        assert tuple(yg.shape) == tuple(y.shape)
        assert rel_err(yg.detach().cpu().numpy(), y.detach().numpy()) < 2e-5, (xs, k)
        assert rel_err(xg.grad.cpu().numpy(), x.grad.numpy()) < 2e-5, (xs, k)
        assert rel_err(wg.grad.cpu().numpy(), w.grad.numpy()) < 2e-5, (xs, k)
        dead = x.grad == 0                                        # voxels outside every window: the gradient there is exactly 0
        untouched += int(dead.sum())
        assert bool((xg.grad.cpu()[dead] == 0).all()), (xs, k)
    assert untouched > 0


# ---- element dropout on (csrc/resnet.hip: elem_drop_scale; the backward recomputes the scale from the flat index) ---------------------
def _record_seeds(monkeypatch):
    from mmnn_sts_amd import ops
    drawn, orig = [], ops.next_seed

    def wrapper():
        drawn.append(orig())
        return drawn[-1]

    monkeypatch.setattr(ops, "next_seed", wrapper)
    return drawn


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_act_dropout_vs_torch(residual, relu, monkeypatch):
    """BatchNormAct3d at drop_p = 0.5, n * c * v = 1050 (not a multiple of the 256-thread blocks): out, running statistics, dx,
    dresidual, dgamma, dbeta against torch fp64 with the restated element mask imposed."""
    from mmnn_sts_amd import ops
    from tests._util import resnet_elem_mask_ref
    torch.manual_seed(7)
    drawn = _record_seeds(monkeypatch)
    shape, c = (2, 5, 3, 5, 7), 5
    x = torch.from_numpy(synth.uniform("bnd/x", shape)).double().requires_grad_(True)
    res = torch.from_numpy(synth.uniform("bnd/r", shape)).double().requires_grad_(True) if residual else None
    gamma = torch.from_numpy(1.0 + 0.5 * synth.uniform("bnd/g", (c,))).double().requires_grad_(True)
    beta = torch.from_numpy(synth.uniform("bnd/b", (c,), 0.3)).double().requires_grad_(True)
    cot = torch.from_numpy(synth.uniform("bnd/c", shape))
    dev = lambda t: t.detach().float().to(DEV).requires_grad_(True) if t is not None else None
    xg, rg, gg, bg = dev(x), dev(res), dev(gamma), dev(beta)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    out = ops.BatchNormAct3d.apply(xg, gg, bg, rm, rv, rg, 0.1, 1e-5, True, relu, 0.5)
    (out * cot.to(DEV)).sum().backward()
    assert len(drawn) == 1 and drawn[0] >= 0
    mask = resnet_elem_mask_ref(drawn[0], x.numel(), 0.5).reshape(shape)
    assert (mask == 0).any() and (mask == 2).any()
    rm64, rv64 = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    y = torch.nn.functional.batch_norm(x, rm64, rv64, gamma, beta, True, 0.1, 1e-5)
    if residual:
        y = y + res
    if relu:
        y = torch.relu(y)
    assert np.array_equal((out.detach().cpu().numpy() == 0) | (y.detach().numpy() == 0), (mask == 0) | (y.detach().numpy() == 0))
    ref = y * torch.from_numpy(mask).double()
    (ref * cot.double()).sum().backward()
    pairs = [("out", out.detach(), ref.detach()), ("running_mean", rm, rm64), ("running_var", rv, rv64), ("dx", xg.grad, x.grad),
             ("dgamma", gg.grad, gamma.grad), ("dbeta", bg.grad, beta.grad)]
    if residual:
        pairs.append(("dresidual", rg.grad, res.grad))
    errs = {k: rel_err(a.cpu().numpy(), b.numpy()) for k, a, b in pairs}
    print("seed", hex(drawn[0]), errs)
    assert max(errs.values()) < 2e-5, errs


def test_r3d18_dropout_train_step_fp64(monkeypatch):
    """r3d_18 end to end at dropout 0.5 (after every stage, fused into the stage's last BN + residual + ReLU): output and all 65
    gradients against the fp64 oracle with the restated element masks imposed, at the tolerances of the dropout-free test above."""
    from mmnn_sts_amd.models import resnet as resnet_mod
    from tests._util import resnet_elem_mask_ref
    torch.manual_seed(3)
    drawn = _record_seeds(monkeypatch)
    stage = []
    orig_bn = resnet_mod._bn

    def bn(x, bnm, relu, residual=None, drop_p=0.0):
        out = orig_bn(x, bnm, relu, residual=residual, drop_p=drop_p)
        if drop_p > 0:
            stage.append((drawn[-1], tuple(out.shape)))
        return out

    monkeypatch.setattr(resnet_mod, "_bn", bn)
    m = _model(dropout=0.5).train()
    shape = (3, 1, 9, 40, 52)
    x = torch.from_numpy(synth.uniform("r3d/x/b", shape))
    y = m(x.to(DEV))
    cot = torch.from_numpy(synth.uniform("r3d/cot/b", tuple(y.shape)))
    (y * cot.to(DEV)).sum().backward()
    assert len(stage) == 4 and len({s for s, _ in stage}) == 4
    masks = {f"layer{i + 1}": torch.from_numpy(resnet_elem_mask_ref(s, int(np.prod(shp)), 0.5).reshape(shp)).double() for i, (s, shp) in enumerate(stage)}
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in synth_sd(R.resnet18_schema(2), "r3d.").items()}
    y64 = R.resnet18_forward(sd, x.double(), True, 0.5, drop_masks=masks)
    (y64 * cot.double()).sum().backward()
    eo = rel_err(y.detach().cpu().numpy(), y64.detach().numpy())
    gl2 = float(torch.sqrt(sum((v.grad ** 2).sum() for v in sd.values() if v.is_floating_point() and v.grad is not None)))
    bad, worst = [], (0.0, "")
    for k, p in m.named_parameters():
        ref = sd[k].grad
        err = float((p.grad.double().cpu() - ref).norm())
        tol = 2e-3 * float(ref.norm()) + 2e-5 * gl2
        worst = max(worst, (err / tol, k))
        if err > tol:
            bad.append((k, err, float(ref.norm())))
    print("output rel err", eo, "worst gradient err/tol", worst)
    assert eo < 1e-4
    assert not bad, (len(bad), gl2, bad[:6])
    sd_dev = m.state_dict()
    for k in sd:
        if "running" in k:
            assert rel_err(sd_dev[k].cpu().numpy(), sd[k].detach().numpy()) < 1e-4, k


# ---- the r3d_18 primitives on their own: geometry edges, eval-mode adjoints, grid-stride second passes ----------------------------------
RELU_MARGIN = 1e-4      # no pre-activation of an fp64 reference may be closer to the ReLU branch point (stream names picked on the CPU)


def test_direct_conv_weight_gradient_accumulates():
    """mmnn_conv3d_backward_weight(accumulate = 1) through ctypes (the autograd function always passes 0): pre-fill + gradient."""
    import ctypes
    from mmnn_sts_amd import _lib, ops
    xs, co, k, s, p = (2, 5, 4, 6, 7), 7, (3, 2, 3), (1, 2, 1), (1, 0, 1)
    x = torch.from_numpy(synth.uniform("conv/acc/x", xs)).double()
    w = torch.from_numpy(synth.uniform("conv/acc/w", (co, xs[1]) + k, 0.3)).double().requires_grad_(True)
    y = torch.nn.functional.conv3d(x, w, None, stride=s, padding=p)
    cot = torch.from_numpy(synth.uniform("conv/acc/c", tuple(y.shape)))
    (y * cot.double()).sum().backward()
    fill = torch.from_numpy(synth.uniform("conv/acc/fill", tuple(w.shape)))
    desc = ops._conv_desc(xs, co, k, s, p)
    L = _lib.lib()
    xg, dy = x.float().to(DEV), cot.to(DEV)
    ws = torch.empty((L.mmnn_conv3d_wgrad_workspace_bytes(ctypes.byref(desc)),), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    plain, acc = torch.full(tuple(w.shape), float("nan"), device=DEV), fill.to(DEV)
    _lib.check(L.mmnn_conv3d_backward_weight(ctypes.byref(desc), xg.data_ptr(), dy.data_ptr(), plain.data_ptr(), ws.data_ptr(), 0, st), "conv3d_backward_weight")
    _lib.check(L.mmnn_conv3d_backward_weight(ctypes.byref(desc), xg.data_ptr(), dy.data_ptr(), acc.data_ptr(), ws.data_ptr(), 1, st), "conv3d_backward_weight")
    assert rel_err(plain.cpu().numpy(), w.grad.numpy()) < 2e-5
    assert rel_err(acc.cpu().numpy(), (fill.double() + w.grad).numpy()) < 2e-5
    assert rel_err(acc.cpu().numpy(), (fill + plain.cpu()).numpy()) <= 2.0 ** -23          # one fp32 addition apart from the plain gradient


def test_direct_conv_filter_bank_beyond_lds_is_refused():
    """128 input channels x 27 taps x a group of 16 output channels = 216 KiB of filters: more than the 160 KiB of LDS.  The forward must
    say so (ValueError through mmnn_last_error) and launch nothing."""
    from mmnn_sts_amd import _lib, ops
    x = torch.zeros(1, 128, 3, 3, 3, device=DEV)
    w = torch.zeros(16, 128, 3, 3, 3, device=DEV)
    with pytest.raises(ValueError, match="160 KiB"):
        ops.Conv3dDirect.apply(x, w, 1, 1)
    assert "filter bank" in _lib.last_error()
    torch.cuda.synchronize()                                      # no launch was queued, so nothing can surface here
    assert float(ops.Conv3dDirect.apply(x[:, :8], w[:, :8].contiguous(), 1, 1).abs().sum()) == 0.0


def _bn_case(tag, shape, relu, residual):
    c = shape[1]
    t = {"x": torch.from_numpy(synth.uniform(f"{tag}/x", shape)), "gamma": torch.from_numpy(synth.uniform(f"{tag}/g", (c,), 0.5, 1.0)),
         "beta": torch.from_numpy(synth.uniform(f"{tag}/b", (c,), 0.3)), "cot": torch.from_numpy(synth.uniform(f"{tag}/c", shape)),
         "rm": torch.from_numpy(synth.uniform(f"{tag}/rm", (c,), 0.3)), "rv": torch.from_numpy(synth.uniform(f"{tag}/rv", (c,), 0.5, 1.0))}
    if residual:
        t["res"] = torch.from_numpy(synth.uniform(f"{tag}/r", shape))
    return t


def _bn_ref(t, training, relu):
    """fp64 batch_norm [+ residual] [+ relu]; returns out, the pre-activation, the leaves and the running statistics after the pass."""
    leaves = {k: t[k].double().requires_grad_(True) for k in ("x", "gamma", "beta", "res") if k in t}
    rm, rv = t["rm"].double().clone(), t["rv"].double().clone()
    pre = torch.nn.functional.batch_norm(leaves["x"], rm, rv, leaves["gamma"], leaves["beta"], training, 0.1, 1e-5)
    if "res" in leaves:
        pre = pre + leaves["res"]
    out = torch.relu(pre) if relu else pre
    (out * t["cot"].double()).sum().backward()
    return out.detach(), pre.detach(), leaves, rm, rv


# v = 130 * 130 = 16900 voxels per channel: more than the launchers' 64 blocks of 256 threads, so every stride loop makes a second pass
BN_CASES = [("bne/s", (2, 5, 3, 5, 7), False, r, s) for r in (False, True) for s in (False, True)]
BN_CASES += [("bne/big/23", (1, 2, 1, 130, 130), True, True, True), ("bne/big/9", (1, 2, 1, 130, 130), False, True, True)]


@pytest.mark.parametrize("tag,shape,training,relu,residual", BN_CASES,
                         ids=[f"v{int(np.prod(c[1][2:]))}-{'train' if c[2] else 'eval'}-relu{int(c[3])}-res{int(c[4])}" for c in BN_CASES])
def test_bn_act_eval_mode_and_second_pass_vs_torch(tag, shape, training, relu, residual):
    """BatchNormAct3d with running statistics (training = False: dx = gamma rstd dz, dgamma = sum dz xhat, dbeta = sum dz, statistics
    bit-unchanged) over relu x residual, and a shape beyond one pass of the grid-stride loops in both modes: out, dx, dresidual, dgamma,
    dbeta against torch fp64."""
    from mmnn_sts_amd import ops
    t = _bn_case(tag, shape, relu, residual)
    ref, pre, leaves, rm64, rv64 = _bn_ref(t, training, relu)
    if relu:
        assert float(pre.abs().min()) >= RELU_MARGIN, f"{tag}: a reference pre-activation lies on the ReLU branch point"
    dev = lambda k: t[k].to(DEV).requires_grad_(True) if k in t else None
    xg, gg, bg, rg = dev("x"), dev("gamma"), dev("beta"), dev("res")
    rm, rv = t["rm"].to(DEV), t["rv"].to(DEV)
    out = ops.BatchNormAct3d.apply(xg, gg, bg, rm, rv, rg, 0.1, 1e-5, training, relu, 0.0)
    (out * t["cot"].to(DEV)).sum().backward()
    pairs = [("out", out.detach(), ref), ("dx", xg.grad, leaves["x"].grad), ("dgamma", gg.grad, leaves["gamma"].grad), ("dbeta", bg.grad, leaves["beta"].grad)]
    if residual:
        pairs.append(("dresidual", rg.grad, leaves["res"].grad))
    if training:
        pairs += [("running_mean", rm, rm64), ("running_var", rv, rv64)]
    else:
        assert torch.equal(rm.cpu(), t["rm"]) and torch.equal(rv.cpu(), t["rv"])
    errs = {k: rel_err(a.cpu().numpy(), b.numpy()) for k, a, b in pairs}
    print(tag, training, relu, residual, errs)
    assert all(e < 2e-5 for e in errs.values()), errs


@pytest.mark.parametrize("n,c,v,o", [(1, 1, (1, 1, 1), 1), (3, 16, (3, 5, 7), 2), (2, 256, (3, 10, 10), 3), (1, 2, (17, 25, 40), 1)])
def test_gap_fc_sigmoid_vs_torch(n, c, v, o):
    """The pooled sigmoid head on its own: out, pooled, dw, db, dx against fp64 at one voxel, 105 voxels (less than a block), the 256-channel
    limit of the kernel's LDS row, and 17000 voxels (beyond the backward's 64 blocks of 256 threads)."""
    from mmnn_sts_amd import ops
    tag = f"gfs/{n}x{c}x{int(np.prod(v))}x{o}"
    x = torch.from_numpy(synth.uniform(f"{tag}/x", (n, c) + v)).double().requires_grad_(True)
    w = torch.from_numpy(synth.uniform(f"{tag}/w", (o, c), 0.5)).double().requires_grad_(True)
    b = torch.from_numpy(synth.uniform(f"{tag}/b", (o,), 0.3)).double().requires_grad_(True)
    cot = torch.from_numpy(synth.uniform(f"{tag}/c", (n, o)))
    pooled = x.mean(dim=(2, 3, 4))
    y = torch.sigmoid(torch.nn.functional.linear(pooled, w, b))
    (y * cot.double()).sum().backward()
    xg, wg, bg = (t.detach().float().to(DEV).requires_grad_(True) for t in (x, w, b))
    yg = ops.GapFcSigmoid.apply(xg, wg, bg)
    pooled_g = yg.grad_fn.saved_tensors[1]
    assert tuple(pooled_g.shape) == (n, c)
    (yg * cot.to(DEV)).sum().backward()
    errs = {"out": rel_err(yg.detach().cpu().numpy(), y.detach().numpy()), "pooled": rel_err(pooled_g.cpu().numpy(), pooled.detach().numpy()),
            "dw": rel_err(wg.grad.cpu().numpy(), w.grad.numpy()), "db": rel_err(bg.grad.cpu().numpy(), b.grad.numpy()),
            "dx": rel_err(xg.grad.cpu().numpy(), x.grad.numpy())}
    print(tag, errs)
    assert all(e < 2e-5 for e in errs.values()), errs


def test_gap_fc_sigmoid_refuses_more_than_256_channels():
    from mmnn_sts_amd import _lib, ops
    x = torch.zeros(1, 257, 1, 2, 2, device=DEV)
    with pytest.raises(ValueError, match="256 channels"):
        ops.GapFcSigmoid.apply(x, torch.zeros(2, 257, device=DEV), torch.zeros(2, device=DEV))
    assert "gap_fc_sigmoid_forward" in _lib.last_error()
    torch.cuda.synchronize()


def test_r3d18_eval_mode_backward_fp64():
    """r3d_18 in .eval() with a backward through it (attribution with respect to the scan, fine-tuning over frozen statistics): output, dx
    and all 65 gradients against the fp64 oracle with running statistics, at the per-tensor rule of the training-mode test; the module's
    statistics and counters do not move.  No ReLU margin is asserted here: of the model's 379904 ReLU inputs about 22 lie within 1e-4 of
    zero in the fp64 reference for this input (11 post-ReLU values in (0, 1e-4)), and as many would for any other; the 2e-3 * |ref| term
    of the rule is what allows for such flips."""
    m = _model().eval()
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    shape = (2, 1, 8, 32, 32)
    x = torch.from_numpy(synth.uniform("r3d/x/eval", shape))
    xg = x.to(DEV).requires_grad_(True)
    y = m(xg)
    cot = torch.from_numpy(synth.uniform("r3d/cot/eval", tuple(y.shape)))
    (y * cot.to(DEV)).sum().backward()
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in synth_sd(R.resnet18_schema(2), "r3d.").items()}
    x64 = x.double().requires_grad_(True)
    y64 = R.resnet18_forward(sd, x64, False)
    (y64 * cot.double()).sum().backward()
    eo = rel_err(y.detach().cpu().numpy(), y64.detach().numpy())
    gl2 = float(torch.sqrt(sum((v.grad ** 2).sum() for v in sd.values() if v.is_floating_point() and v.grad is not None)))
    bad, worst = [], (0.0, "")
    for k, p in m.named_parameters():
        ref = sd[k].grad
        err = float((p.grad.double().cpu() - ref).norm())
        tol = 2e-3 * float(ref.norm()) + 2e-5 * gl2
        worst = max(worst, (err / tol, k))
        if err > tol:
            bad.append((k, err, float(ref.norm())))
    ex = float((xg.grad.double().cpu() - x64.grad).norm()) / (2e-3 * float(x64.grad.norm()) + 2e-5 * gl2)
    print("output rel err", eo, "worst gradient err/tol", worst, "dx err/tol", ex)
    assert eo < 1e-4
    assert not bad, (len(bad), gl2, bad[:6])
    assert len(list(m.named_parameters())) == 65
    assert ex < 1.0
    after = m.state_dict()
    assert len(before) == 63 and all(torch.equal(after[k], v) for k, v in before.items())
