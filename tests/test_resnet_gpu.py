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
             ((1, 8, 7, 11, 9), 16, (3, 3, 3), 2, 1), ((2, 8, 7, 11, 9), 16, (1, 1, 1), 2, 0), ((3, 5, 4, 6, 7), 19, (2, 3, 1), (1, 2, 3), (1, 0, 2))]
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
