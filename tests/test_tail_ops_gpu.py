"""The tail kernels (csrc/tail.hip: MLP stacks, fusion heads, small linear, BCE with logits, GAP + linear) on their own, each against a
plain fp64 restatement written here from torch CPU ops -- both BatchNorm modes, grid-stride second passes, NULL optional buffers and
the `accumulate = 1` branches that the model-level goldens never reach.

Bars: rel_err < 2e-5 per tensor (the fp32-VALU-against-fp64 bar of tests/test_resnet_gpu.py), rtol 2e-5 / atol 1e-7 element-wise for BCE
(tests/test_fusion_gpu.py).  Every reduction here is at most 1100 fp32 terms.  The fp64 reference never sits on a ReLU branch: each
case asserts that no pre-activation of the reference is within 1e-4 of zero (the stream names below were picked on the CPU for that),
and no element is left out of a comparison."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from oracle import synth
from tests._util import N_CLIN, rel_err, synth_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-5
RELU_MARGIN = 1e-4
BN_MOMENTUM, BN_EPS = 0.1, 1e-5


def _u(name, shape, scale=1.0, offset=0.0):
    return torch.from_numpy(synth.uniform(name, shape, scale, offset))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _assert_off_branch(pres, what):
    worst = min(float(p.detach().abs().min()) for p in pres)
    assert worst >= RELU_MARGIN, f"{what}: a reference pre-activation lies {worst:.3e} from the ReLU branch point"


def _check(errs, bar=BAR):
    bad = {k: v for k, v in errs.items() if not v < bar}          # (a NaN -- an element nobody wrote -- is not below the bar)
    print("worst rel_err", max(errs.items(), key=lambda kv: kv[1]), "of", len(errs), "tensors")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# MLP stacks
# ---------------------------------------------------------------------------------------------------------------------------------
MLP_SCHEMA = R.mlp_schema(N_CLIN, 2, 12)
MLP_LAYERS = [("backbone", i) for i in range(5)] + [("features", 5)]
MLP_PARAM_KEYS = [f"{s}.{m}{i}.{leaf}" for s, i in MLP_LAYERS for m, leaf in (("dense", "weight"), ("dense", "bias"), ("bn", "weight"), ("bn", "bias"))]
MLP_RUN_KEYS = [f"{s}.bn{i}.{leaf}" for s, i in MLP_LAYERS for leaf in ("running_mean", "running_var", "num_batches_tracked")]
# input stream per (mode, batch size): the first index at which no pre-activation of the fp64 reference is within 1e-4 of zero
MLP_X_STREAM = {("train", 300): 5, ("eval", 37): 3, ("eval", 300): 229}


def mlp_sd():
    return synth_sd(MLP_SCHEMA, "tailmlp.")


def mlp_x(mode, n):
    return _u(f"tail/mlp/x/{mode}/{n}/{MLP_X_STREAM.get((mode, n), 0)}", (n, N_CLIN))


def mlp_ref(sd, x, training, layers=MLP_LAYERS, dtype=torch.float64):
    """[Linear -> BatchNorm1d -> ReLU] per layer (dropout_prob = 0, so the order of drop and relu does not matter).  Returns the output, the
    leaves {key: tensor} (x under "x", the dense outputs z under "z{i}" with their gradients retained; the running statistics are updated
    in place) and the BN outputs that feed the ReLUs."""
    p = {k: v.detach().clone().to(dtype) if v.is_floating_point() else v.clone() for k, v in sd.items()}
    for k in MLP_PARAM_KEYS:
        p[k].requires_grad_(True)
    p["x"] = x.detach().clone().to(dtype).requires_grad_(True)
    h, pres = p["x"], []
    for s, i in layers:
        z = F.linear(h, p[f"{s}.dense{i}.weight"], p[f"{s}.dense{i}.bias"])
        z.retain_grad()
        p[f"z{i}"] = z
        y = F.batch_norm(z, p[f"{s}.bn{i}.running_mean"], p[f"{s}.bn{i}.running_var"], p[f"{s}.bn{i}.weight"], p[f"{s}.bn{i}.bias"],
                         training, BN_MOMENTUM, BN_EPS)
        pres.append(y)
        h = F.relu(y)
    return h, p, pres


def mlp_grad_err(k, got, leaves, training):
    """rel_err of one parameter gradient.  A dense bias in front of a training-mode BatchNorm has the gradient sum_n dz[n, o] = 0 exactly
    (the norm removes the batch mean), so the reference holds rounding noise only and is no yardstick: the error of such a sum is taken
    against the size of what is summed, max_o sum_n |dz[n, o]|, as every fp32 summation bound is stated."""
    ref = leaves[k].grad
    if training and ".dense" in k and k.endswith(".bias"):
        dz = leaves["z" + k.split(".dense")[1][0]].grad
        return float((got.double().cpu() - ref).abs().max() / dz.abs().sum(dim=0).max())
    return rel_err(got.cpu().numpy(), ref.numpy())


# BatchNorm over N = 2 rows in training mode is degenerate: xhat = +-(1 - eps / 2 d^2) whatever the input, and every gradient in front of
# the norm is proportional to 1 - xhat^2 ~ 1e-4, a difference of two fp32 numbers near 1.  torch's own fp32 evaluation of mlp_ref on the
# CPU is 4.3e-4 off the fp64 one there (worst tensor: dx; 24 of the 26 tensors are between 1.0e-4 and 4.3e-4; every other case of
# MLP_CASES: <= 7.9e-6).  With the factor 4 for another summation order the bar of that one case is 1.72e-3.
MLP_BAR = {("train", 2): 4 * 4.31e-4}
MLP_CASES = [("train", 2), ("train", 3), ("train", 37), ("train", 300), ("eval", 1), ("eval", 2), ("eval", 3), ("eval", 37), ("eval", 300)]


@pytest.mark.parametrize("mode,n", MLP_CASES)
def test_mlp_stack_vs_fp64(mode, n):
    """MLP(N_CLIN, 2, 12) with dropout off, both stacks, batch and running statistics: features, dx and the 24 parameter gradients.  N = 300
    gives N * O = 9600 elements to the 256 threads of the one block.  Eval mode: the adjoint of y = gamma (z - rmean) rstd + beta is
    dz = gamma rstd g with dgamma = sum g xhat, dbeta = sum g, and nothing of the module's state moves."""
    from mmnn_sts_amd.models.mlp import MLP
    training = mode == "train"
    sd = mlp_sd()
    x = mlp_x(mode, n)
    cot = _u(f"tail/mlp/cot/{n}", (n, 12))
    ref, leaves, pres = mlp_ref(sd, x, training)
    _assert_off_branch(pres, f"mlp {mode} n={n}")
    (ref * cot.double()).sum().backward()
    m = MLP(N_CLIN, 2, 12, dropout_prob=0.0)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train(training)
    before = {k: v.clone() for k, v in m.state_dict().items() if k in MLP_RUN_KEYS}
    xg = x.to(DEV).requires_grad_(True)
    f = m.features(m.backbone(xg))
    (f * cot.to(DEV)).sum().backward()
    params = dict(m.named_parameters())
    errs = {"features": rel_err(f.detach().cpu().numpy(), ref.detach().numpy()), "dx": rel_err(xg.grad.cpu().numpy(), leaves["x"].grad.numpy())}
    for k in MLP_PARAM_KEYS:
        errs[k] = mlp_grad_err(k, params[k].grad, leaves, training)
    assert len(errs) == 26 and params["output_head.dense6.weight"].grad is None
    after = m.state_dict()
    if training:
        for k in MLP_RUN_KEYS:
            if k.endswith("num_batches_tracked"):
                assert int(after[k]) == 1, k
            else:
                errs[k] = rel_err(after[k].cpu().numpy(), leaves[k].numpy())
    else:
        for k in MLP_RUN_KEYS:
            assert torch.equal(after[k], before[k]), k             # bit-unchanged
    _check(errs, MLP_BAR.get((mode, n), BAR))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_mlp_stack_without_input_gradient(mode):
    """`x` does not require grad: the kernel gets dx = NULL and must still produce every parameter gradient."""
    from mmnn_sts_amd.models.mlp import MLP
    training, n = mode == "train", 37
    sd = mlp_sd()
    x = mlp_x(mode, n)
    cot = _u(f"tail/mlp/cot/{n}", (n, 12))
    ref, leaves, pres = mlp_ref(sd, x, training)
    _assert_off_branch(pres, f"mlp {mode} n={n}")
    (ref * cot.double()).sum().backward()
    m = MLP(N_CLIN, 2, 12, dropout_prob=0.0)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train(training)
    xg = x.to(DEV)
    f = m.features(m.backbone(xg))
    (f * cot.to(DEV)).sum().backward()
    assert xg.grad is None
    params = dict(m.named_parameters())
    _check({k: mlp_grad_err(k, params[k].grad, leaves, training) for k in MLP_PARAM_KEYS})


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_mlp_backward_accumulates(mode):
    """mmnn_mlp_backward(accumulate = 1) on the five-layer backbone stack, driven through ctypes (the autograd wrapper always passes 0): the
    pre-filled gradient buffers come back as pre-fill + gradient; dx is overwritten either way."""
    from mmnn_sts_amd import _lib, ops
    training, n = mode == "train", 37
    layers = MLP_LAYERS[:5]
    keys = [k for k in MLP_PARAM_KEYS if k.startswith("backbone.")]
    sd = mlp_sd()
    x = mlp_x(mode, n)
    cot = _u(f"tail/mlp/acc/cot/{n}", (n, 8))
    ref, leaves, pres = mlp_ref(sd, x, training, layers)
    _assert_off_branch(pres, f"mlp backbone {mode} n={n}")
    (ref * cot.double()).sum().backward()
    dev = {k: v.to(DEV) for k, v in sd.items()}
    dims_in = [dev[f"backbone.dense{i}.weight"].shape[1] for i in range(5)]
    dims_out = [dev[f"backbone.dense{i}.weight"].shape[0] for i in range(5)]
    desc = ops._mlp_desc(n, dims_in, dims_out, [True, False, False, False, False], 0.0, BN_EPS, BN_MOMENTUM, 0, training, 0)
    L = _lib.lib()
    xg, dy = x.to(DEV), cot.to(DEV)
    saved = torch.empty((L.mmnn_mlp_saved_floats(ctypes.byref(desc)),), device=DEV)
    out = torch.empty((n, 8), device=DEV)
    scratch = torch.empty((2 * n * max(dims_in + dims_out),), device=DEV)

    def params(grads):
        pp = _lib.MlpParams()
        for i in range(5):
            pp.weight[i], pp.bias[i] = dev[f"backbone.dense{i}.weight"].data_ptr(), dev[f"backbone.dense{i}.bias"].data_ptr()
            pp.gamma[i], pp.beta[i] = dev[f"backbone.bn{i}.weight"].data_ptr(), dev[f"backbone.bn{i}.bias"].data_ptr()
            pp.running_mean[i], pp.running_var[i] = dev[f"backbone.bn{i}.running_mean"].data_ptr(), dev[f"backbone.bn{i}.running_var"].data_ptr()
            pp.grad_weight[i], pp.grad_bias[i], pp.grad_gamma[i], pp.grad_beta[i] = (grads[keys[4 * i + j]].data_ptr() for j in range(4))
        return pp

    plain = {k: torch.full_like(dev[k], float("nan")) for k in keys}
    _lib.check(L.mmnn_mlp_forward(ctypes.byref(desc), ctypes.byref(params(plain)), xg.data_ptr(), out.data_ptr(), saved.data_ptr(), _stream()), "mlp_forward")
    dx = torch.full_like(xg, float("nan"))
    _lib.check(L.mmnn_mlp_backward(ctypes.byref(desc), ctypes.byref(params(plain)), xg.data_ptr(), saved.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                                   scratch.data_ptr(), 0, _stream()), "mlp_backward")
    fill = {k: _u(f"tail/mlp/acc/fill/{k}", tuple(dev[k].shape)) for k in keys}
    acc = {k: fill[k].to(DEV) for k in keys}
    dx2 = torch.full_like(xg, 3.0)
    _lib.check(L.mmnn_mlp_backward(ctypes.byref(desc), ctypes.byref(params(acc)), xg.data_ptr(), saved.data_ptr(), dy.data_ptr(), dx2.data_ptr(),
                                   scratch.data_ptr(), 1, _stream()), "mlp_backward")
    errs = {"out": rel_err(out.cpu().numpy(), ref.detach().numpy()), "dx": rel_err(dx.cpu().numpy(), leaves["x"].grad.numpy())}
    assert torch.equal(dx, dx2)
    for k in keys:
        errs[k] = mlp_grad_err(k, plain[k], leaves, training)
        errs["acc/" + k] = rel_err(acc[k].cpu().numpy(), (fill[k].double() + leaves[k].grad).numpy())
        # against the device's own gradient the sum is one fp32 addition: at most half an ulp of the largest element apart
        assert rel_err(acc[k].cpu().numpy(), (fill[k] + plain[k].cpu()).numpy()) <= 2.0 ** -23, k
    _check(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# fusion heads
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 1, 1), (2, 12, 2), (5, 12, 3), (37, 7, 5), (300, 12, 2)]
HEAD_NAMES = ("fi", "fc", "wf", "bf", "wi", "bi", "wc", "bc")


def heads_inputs(n, f, c):
    """Every operand from a stream of its own (a swapped pair -- fi / fc, wi / wc -- cannot pass)."""
    tag = f"tail/heads/{n}x{f}x{c}"
    shapes = {"fi": (n, f), "fc": (n, f), "wf": (c, 2 * f), "bf": (c,), "wi": (c, f), "bi": (c,), "wc": (c, f), "bc": (c,)}
    return {k: _u(f"{tag}/{k}", s, 1.0 if k in ("fi", "fc") else 0.5) for k, s in shapes.items()}


def heads_ref(t, blend):
    out = F.linear(torch.cat([t["fi"], t["fc"]], 1), t["wf"], t["bf"])
    if not blend:
        return out
    return torch.stack((out, F.linear(t["fi"], t["wi"], t["bi"]), F.linear(t["fc"], t["wc"], t["bc"])), 0)


@pytest.mark.parametrize("blend", [False, True])
@pytest.mark.parametrize("n,f,c", HEAD_SHAPES)
def test_fusion_heads_vs_fp64(n, f, c, blend):
    """out and all eight gradients; (300, 12, 2) gives 3 * n * c = 1800 outputs and n * f = 3600 feature gradients to the 256 threads of the
    one block.  Without blend the per-modality heads are not part of the graph: their gradients are None."""
    from mmnn_sts_amd import ops
    inp = heads_inputs(n, f, c)
    t64 = {k: v.double().requires_grad_(True) for k, v in inp.items()}
    ref = heads_ref(t64, blend)
    cot = _u(f"tail/heads/cot/{n}x{f}x{c}/{int(blend)}", tuple(ref.shape))
    (ref * cot.double()).sum().backward()
    tg = {k: v.to(DEV).requires_grad_(True) for k, v in inp.items()}
    out = ops.FusionHeads.apply(*(tg[k] for k in HEAD_NAMES), blend)
    assert tuple(out.shape) == tuple(ref.shape)
    (out * cot.to(DEV)).sum().backward()
    errs = {"out": rel_err(out.detach().cpu().numpy(), ref.detach().numpy())}
    for k in HEAD_NAMES:
        if not blend and k in ("wi", "bi", "wc", "bc"):
            assert tg[k].grad is None and t64[k].grad is None, k
            continue
        errs["d" + k] = rel_err(tg[k].grad.cpu().numpy(), t64[k].grad.numpy())
    assert len(errs) == (9 if blend else 5)
    _check(errs)


def test_fusion_heads_backward_accumulates():
    """mmnn_fusion_heads_backward(accumulate = 1) through ctypes at (5, 12, 3) with blend: the six parameter gradients come back as
    pre-fill + gradient, the two feature gradients are overwritten."""
    from mmnn_sts_amd import _lib
    n, f, c = 5, 12, 3
    inp = heads_inputs(n, f, c)
    t64 = {k: v.double().requires_grad_(True) for k, v in inp.items()}
    ref = heads_ref(t64, True)
    cot = _u(f"tail/heads/cot/{n}x{f}x{c}/1", tuple(ref.shape))
    (ref * cot.double()).sum().backward()
    tg = {k: v.to(DEV) for k, v in inp.items()}
    dout = cot.to(DEV)
    fill = {k: _u(f"tail/heads/fill/{k}", tuple(inp[k].shape)) for k in HEAD_NAMES}
    L = _lib.lib()
    res = {}
    for accumulate in (0, 1):
        g = {k: (fill[k].to(DEV) if accumulate else torch.full_like(tg[k], float("nan"))) for k in HEAD_NAMES}
        _lib.check(L.mmnn_fusion_heads_backward(n, f, c, 1, tg["fi"].data_ptr(), tg["fc"].data_ptr(), tg["wf"].data_ptr(), tg["wi"].data_ptr(),
                                                tg["wc"].data_ptr(), dout.data_ptr(), g["fi"].data_ptr(), g["fc"].data_ptr(), g["wf"].data_ptr(),
                                                g["bf"].data_ptr(), g["wi"].data_ptr(), g["bi"].data_ptr(), g["wc"].data_ptr(), g["bc"].data_ptr(),
                                                accumulate, _stream()), "fusion_heads_backward")
        res[accumulate] = {k: v.cpu() for k, v in g.items()}
    errs = {}
    for k in HEAD_NAMES:
        errs["d" + k] = rel_err(res[0][k].numpy(), t64[k].grad.numpy())
        if k in ("fi", "fc"):
            assert torch.equal(res[1][k], res[0][k]), k
        else:
            errs["acc/d" + k] = rel_err(res[1][k].numpy(), (fill[k].double() + t64[k].grad).numpy())
            assert rel_err(res[1][k].numpy(), (fill[k] + res[0][k]).numpy()) <= 2.0 ** -23, k
    _check(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# small linear
# ---------------------------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(1, 1, 1), (3, 12, 2), (1100, 12, 16), (1100, 16, 3)]


def linear_inputs(n, d, o):
    tag = f"tail/linear/{n}x{d}x{o}"
    return _u(f"{tag}/x", (n, d)), _u(f"{tag}/w", (o, d), 0.5), _u(f"{tag}/b", (o,), 0.3), _u(f"{tag}/cot", (n, o))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n,d,o", LINEAR_SHAPES)
def test_small_linear_vs_fp64(n, d, o, bias):
    """y, dx, dw, db.  The launchers cap their grids at 64 blocks of 256 threads = 16384 elements per pass: n * o = 17600 (third shape)
    sends the forward, n * d = 17600 (fourth shape) the backward into a second pass of the grid-stride loop."""
    from mmnn_sts_amd import ops
    x, w, b, cot = linear_inputs(n, d, o)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if bias else None
    ref = F.linear(x64, w64, b64)
    (ref * cot.double()).sum().backward()
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True) if bias else None
    y = ops.SmallLinear.apply(xg, wg, bg)
    (y * cot.to(DEV)).sum().backward()
    errs = {"y": rel_err(y.detach().cpu().numpy(), ref.detach().numpy()), "dx": rel_err(xg.grad.cpu().numpy(), x64.grad.numpy()),
            "dw": rel_err(wg.grad.cpu().numpy(), w64.grad.numpy())}
    if bias:
        errs["db"] = rel_err(bg.grad.cpu().numpy(), b64.grad.numpy())
    _check(errs)


def test_small_linear_null_dx_and_accumulate():
    """`x` without a gradient (dx = NULL) through the autograd function, and accumulate = 1 (with and without db) through ctypes, at
    (1100, 16, 3) so that the skipped dx store sits inside a two-pass loop."""
    from mmnn_sts_amd import _lib, ops
    n, d, o = 1100, 16, 3
    x, w, b, cot = linear_inputs(n, d, o)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    (F.linear(x64, w64, b64) * cot.double()).sum().backward()
    xg, wg, bg = x.to(DEV), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    (ops.SmallLinear.apply(xg, wg, bg) * cot.to(DEV)).sum().backward()
    assert xg.grad is None
    errs = {"dw/no-dx": rel_err(wg.grad.cpu().numpy(), w64.grad.numpy()), "db/no-dx": rel_err(bg.grad.cpu().numpy(), b64.grad.numpy())}
    L = _lib.lib()
    dy = cot.to(DEV)
    fw, fb = _u("tail/linear/fill/w", (o, d)), _u("tail/linear/fill/b", (o,))
    for with_db in (True, False):
        dx, dw, db = torch.full_like(xg, float("nan")), fw.to(DEV), fb.to(DEV)
        _lib.check(L.mmnn_linear_backward(n, d, o, xg.data_ptr(), wg.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                          db.data_ptr() if with_db else None, 1, _stream()), "linear_backward")
        errs[f"acc/dx/{with_db}"] = rel_err(dx.cpu().numpy(), x64.grad.numpy())
        errs[f"acc/dw/{with_db}"] = rel_err(dw.cpu().numpy(), (fw.double() + w64.grad).numpy())
        assert rel_err(dw.cpu().numpy(), (fw + wg.grad.cpu()).numpy()) <= 2.0 ** -23
        if with_db:
            errs["acc/db"] = rel_err(db.cpu().numpy(), (fb.double() + b64.grad).numpy())
            assert rel_err(db.cpu().numpy(), (fb + bg.grad.cpu()).numpy()) <= 2.0 ** -23
        else:
            assert torch.equal(db.cpu(), fb)                       # db = NULL: nothing written
    _check(errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# BCE with logits
# ---------------------------------------------------------------------------------------------------------------------------------
BCE_PLANTED = (0.0, 1e-4, -1e-4, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0)


def bce_inputs(rows, c, soft):
    """Logits uniform in [-6, 6) with the planted values at the front of every class column's share, targets hard {0, 1} or soft [0, 1),
    positive-class weights in [0.5, 3.5)."""
    tag = f"tail/bce/{rows}x{c}/{int(soft)}"
    x = _u(f"{tag}/x", (rows, c), 6.0).clone()
    flat = x.view(-1)
    k = len(BCE_PLANTED)
    flat[:2 * k] = torch.tensor(BCE_PLANTED + BCE_PLANTED[::-1])       # consecutive elements: every class and both target kinds meet them
    if rows * c > 4 * k:
        flat[-k:] = torch.tensor(BCE_PLANTED)                           # ... and the last pass of the loop
    u = _u(f"{tag}/y", (rows, c), 0.5, 0.5)
    y = u if soft else (u > 0.5).float()
    pw = _u(f"tail/bce/pw/{c}", (c,), 1.5, 2.0)
    return x, y, pw


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("rows,c", [(37, 1), (37, 3), (87500, 3)])
def test_bce_logits_vs_fp64(rows, c, weighted, soft):
    """Loss and d loss / d logits element by element against F.binary_cross_entropy_with_logits in fp64.  87500 * 3 = 262500 elements
    exceed the launcher's 1024 blocks of 256 threads (262144), so the grid-stride loop makes a second pass."""
    from mmnn_sts_amd import ops
    x, y, pw = bce_inputs(rows, c, soft)
    for v in BCE_PLANTED:
        assert (x == v).any()
    x64 = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(x64, y.double(), pos_weight=pw.double() if weighted else None, reduction="none")
    ref.sum().backward()
    xg = x.to(DEV).requires_grad_(True)
    loss = ops.BceLogits.apply(xg, y.to(DEV), pw.to(DEV) if weighted else None)
    loss.sum().backward()
    assert torch.isfinite(loss).all() and torch.isfinite(xg.grad).all()
    np.testing.assert_allclose(loss.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), x64.grad.numpy(), rtol=2e-5, atol=1e-7)


def test_bce_logits_without_gradient_and_errors():
    """Logits that do not require grad: dloss_dlogits = NULL, the loss is still complete.  total % c != 0 and the other bad arguments come
    back as status 1 with a message (ValueError), before any launch."""
    from mmnn_sts_amd import _lib, ops
    x, y, pw = bce_inputs(37, 3, True)
    ref = F.binary_cross_entropy_with_logits(x.double(), y.double(), pos_weight=pw.double(), reduction="none")
    loss = ops.BceLogits.apply(x.to(DEV), y.to(DEV), pw.to(DEV))
    assert not loss.requires_grad
    np.testing.assert_allclose(loss.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=1e-7)
    L = _lib.lib()
    xg, yg = x.to(DEV), y.to(DEV)
    out = torch.full((37, 3), 7.0, device=DEV)
    for total, c in ((7, 3), (110, 3), (0, 3), (6, 0)):
        rc = L.mmnn_bce_logits(total, c, xg.data_ptr(), yg.data_ptr(), None, out.data_ptr(), None, _stream())
        assert rc == 1 and "bce_logits" in _lib.last_error(), (total, c)
        with pytest.raises(ValueError, match="bce_logits"):
            _lib.check(rc, "bce_logits")
    assert bool((out == 7.0).all())                                    # nothing was launched
    with pytest.raises(ValueError, match="pos_weight"):
        ops.BceLogits.apply(xg, yg, torch.ones(2, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------------
# GAP + linear (DenseNet.features)
# ---------------------------------------------------------------------------------------------------------------------------------
GAP_SHAPE = (3, 40, (2, 3, 5), 12)


def gap_inputs():
    n, c, dhw, f = GAP_SHAPE
    return (_u("tail/gap/h", (n, c) + dhw), _u("tail/gap/w", (f, c), 0.2), _u("tail/gap/b", (f,), 0.1), _u("tail/gap/cot", (n, f)))


def gap_ref(h, w, b, cot):
    h64, w64, b64 = (t.double().requires_grad_(True) for t in (h, w, b))
    assert float(h64.detach().abs().min()) >= RELU_MARGIN, "gap: an input lies on the ReLU branch point"
    ref = F.linear(torch.relu(h64).mean(dim=(2, 3, 4)), w64, b64)
    (ref * cot.double()).sum().backward()
    return ref.detach(), h64.grad, w64.grad, b64.grad


def test_gap_linear_eval_backward_ignores_dropout():
    """training = False with p = 0.5: the flag must turn the element dropout off in the forward and in the backward."""
    from mmnn_sts_amd import ops
    h, w, b, cot = gap_inputs()
    ref, dh, dw, db = gap_ref(h, w, b, cot)
    hg, wg, bg = (t.to(DEV).requires_grad_(True) for t in (h, w, b))
    out = ops.GapLinear.apply(hg, wg, bg, 0.5, False)
    (out * cot.to(DEV)).sum().backward()
    _check({"out": rel_err(out.detach().cpu().numpy(), ref.numpy()), "dh": rel_err(hg.grad.cpu().numpy(), dh.numpy()),
            "dw": rel_err(wg.grad.cpu().numpy(), dw.numpy()), "db": rel_err(bg.grad.cpu().numpy(), db.numpy())})


def test_gap_linear_backward_accumulates():
    """mmnn_gap_linear_backward(accumulate = 1) through ctypes: dw and db come back as pre-fill + gradient, dh is overwritten."""
    from mmnn_sts_amd import _lib
    n, c, dhw, f = GAP_SHAPE
    v = int(np.prod(dhw))
    h, w, b, cot = gap_inputs()
    ref, dh, dw, db = gap_ref(h, w, b, cot)
    L = _lib.lib()
    hg, wg, bg, dout = (t.to(DEV) for t in (h, w, b, cot))
    pooled, out = torch.empty((n, c), device=DEV), torch.empty((n, f), device=DEV)
    _lib.check(L.mmnn_gap_linear_forward(n, c, v, f, hg.data_ptr(), wg.data_ptr(), bg.data_ptr(), pooled.data_ptr(), out.data_ptr(), 0.0, 0, 1,
                                         _stream()), "gap_linear_forward")
    fw, fb = _u("tail/gap/fill/w", (f, c)), _u("tail/gap/fill/b", (f,))
    res = {}
    for accumulate in (0, 1):
        gw = fw.to(DEV) if accumulate else torch.full_like(wg, float("nan"))
        gb = fb.to(DEV) if accumulate else torch.full_like(bg, float("nan"))
        gh = torch.full_like(hg, 3.0)
        _lib.check(L.mmnn_gap_linear_backward(n, c, v, f, hg.data_ptr(), wg.data_ptr(), pooled.data_ptr(), dout.data_ptr(), gw.data_ptr(),
                                              gb.data_ptr(), gh.data_ptr(), 0.0, 0, 1, accumulate, _stream()), "gap_linear_backward")
        res[accumulate] = (gh.cpu(), gw.cpu(), gb.cpu())
    assert torch.equal(res[0][0], res[1][0])
    assert rel_err(res[1][1].numpy(), (fw + res[0][1]).numpy()) <= 2.0 ** -23 and rel_err(res[1][2].numpy(), (fb + res[0][2]).numpy()) <= 2.0 ** -23
    _check({"out": rel_err(out.cpu().numpy(), ref.numpy()), "dh": rel_err(res[0][0].numpy(), dh.numpy()),
            "dw": rel_err(res[0][1].numpy(), dw.numpy()), "db": rel_err(res[0][2].numpy(), db.numpy()),
            "acc/dw": rel_err(res[1][1].numpy(), (fw.double() + dw).numpy()), "acc/db": rel_err(res[1][2].numpy(), (fb.double() + db).numpy())})
