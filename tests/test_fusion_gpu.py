"""Parity of the drop-in Python API (models.*, losses.*, utils.*) running on the HIP kernels: golden vectors produced
by the reference's own classes (tests/golden), the fp64 oracle, and the known answers of the Cox loss."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import restatement as R
from oracle import synth
from tests._util import N_CLIN, clin_in, image_in, labels, load_golden, rel_err, stat3, synth_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _load(module, schema, prefix):
    sd = synth_sd(schema, prefix)
    module.load_state_dict(sd, strict=True)
    return module


def _zero_dropout(m):
    for mod in m.modules():
        if mod.__class__.__name__.startswith("Dropout"):
            mod.p = 0.0
    for mod in m.modules():
        if hasattr(mod, "cfg") and isinstance(getattr(mod, "cfg"), dict) and "dropout_prob" in mod.cfg:
            mod.cfg["dropout_prob"] = 0.0
    return m


def _fusion(blend, dropout=0.0):
    from mmnn_sts_amd.models.densenet import DenseNet121
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    img = DenseNet121(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=dropout)
    mm = MultiModalModel(img, [f"p{i}" for i in range(N_CLIN)], 2, 12, blend=blend)
    _load(mm, R.multimodal_schema(R.DenseNetCfg(), N_CLIN, 2, 12), "fusion.")
    return mm.to(DEV)


def test_cox_known_answers():
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    g = load_golden("g6_blender.npz")
    t = lambda a, dt=None: torch.tensor(a, device=DEV, dtype=dt)
    k1 = CoxPH(t([.3, -.2, .1, .4]), t([1, 0, 1, 1]), t([100, 250, 300, 50]))
    assert abs(k1.item() - 1.04063249) < 2e-6                                   # SURVEY 8(c) KAT1, as the reference calls it
    k1i = CoxPH(t([.3, -.2, .1, .4]), t([1, 0, 1, 1]), t([100, 250, 300, 50]), intended_order=True)
    assert abs(k1i.item() - 0.68245322) < 2e-6
    P = t([[.3, -.2], [.1, .4], [-.5, .2], [0, .7]])
    E = t([[1, 0], [0, 1], [1, 1], [0, 0]])
    D = t([[100, 250], [300, 50], [20, 400], [75, 75]])
    assert abs(surv_criterion(CoxPH, P, E, D, DEV).item() - 1.85874867) < 2e-6    # KAT2
    preds = t([[[.3, -.2], [.1, .4]], [[.5, 0], [-.1, .2]], [[0, .1], [.2, -.3]]])
    ev, du = labels(2)
    gb = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion)
    loss, sel = gb.computeLoss(preds, ev.to(DEV), du.to(DEV))
    assert abs(loss.item() - 1.26084220) < 2e-6 and abs(sel.item() - 1.46317768) < 2e-6   # KAT3
    np.testing.assert_allclose(gb.computeLossSurv(preds, ev.to(DEV), du.to(DEV), reduceToHeads=True).cpu().numpy(), g["kat3_heads"], rtol=2e-6)


def test_cox_gradient_vs_oracle():
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    for n in (2, 8, 16, 37):
        p = torch.from_numpy(synth.uniform(f"cox/p{n}", (3, n, 2))).double().requires_grad_(True)
        ev = torch.from_numpy((synth.uniform(f"cox/e{n}", (n, 2)) > -0.3).astype(np.int64))
        ev[0] = 1
        du = torch.from_numpy((1 + np.floor((synth.uniform(f"cox/d{n}", (n, 2)) * .5 + .5) * 2998)).astype(np.int64))
        b = R.Blender()
        b.weights = torch.tensor([0.5, 0.3, 0.2], dtype=torch.float64)
        loss, _ = b.compute_loss(p, ev, du)
        loss.backward()
        pg = p.detach().float().to(DEV).requires_grad_(True)
        gb = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion)
        gb.weights = torch.tensor([0.5, 0.3, 0.2], device=DEV)
        lg, _ = gb.computeLoss(pg, ev.to(DEV), du.to(DEV))
        lg.backward()
        assert abs(lg.item() - loss.item()) < 2e-5 * abs(loss.item()), n
        assert rel_err(pg.grad.cpu().numpy(), p.grad.numpy()) < 2e-5, n


def test_blender_update_sequence():
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    g = load_golden("g6_blender.npz")
    gb = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion)
    mk = lambda a: torch.from_numpy(a).to(DEV)
    for it in range(3):
        tp = mk(synth.uniform(f"gb/train/{it}", (3, 12, 2)))
        vp = mk(synth.uniform(f"gb/val/{it}", (3, 10, 2)))
        te = mk((synth.uniform("gb/te", (12, 2)) > -0.2).astype(np.int64))
        ve = mk((synth.uniform("gb/ve", (10, 2)) > -0.2).astype(np.int64))
        td = mk((1 + np.floor((synth.uniform("gb/td", (12, 2)) * .5 + .5) * 2998)).astype(np.int64))
        vd = mk((1 + np.floor((synth.uniform("gb/vd", (10, 2)) * .5 + .5) * 2998)).astype(np.int64))
        gb.updateWeights(tp, te, td, vp, ve, vd)
        np.testing.assert_allclose(gb.weights.cpu().numpy(), g["upd_weights"][it], rtol=2e-4, atol=1e-6)
        np.testing.assert_allclose(gb.ltn.cpu().numpy(), g["upd_losses"][it][0], rtol=2e-6)
    assert len(gb.history) == 3


@pytest.mark.parametrize("n", [2, 8])
def test_mlp_golden(n):
    from mmnn_sts_amd.models.mlp import MLP
    g = load_golden("g1_mlp.npz")
    sch = R.mlp_schema(N_CLIN, 2, 12)
    m = _zero_dropout(_load(MLP(N_CLIN, 2, 12), sch, "mlp.")).to(DEV)
    x = clin_in(n).to(DEV)
    m.eval()
    with torch.no_grad():
        assert rel_err(m(x).cpu().numpy(), g[f"eval_out_n{n}"]) < 2e-5
    m.train()
    f = m.features(m.backbone(x))
    y = m.output_head(f)
    (y * torch.from_numpy(synth.uniform("mlp/cot", tuple(y.shape))).to(DEV)).sum().backward()
    assert rel_err(f.detach().cpu().numpy(), g[f"train_feat_n{n}"]) < 2e-5
    assert rel_err(y.detach().cpu().numpy(), g[f"train_out_n{n}"]) < 2e-5
    sd = m.state_dict()
    for k in sch:
        if "running" in k:
            assert rel_err(sd[k].cpu().numpy(), g[f"run_n{n}/{k}"]) < 2e-5, k
    for k, p in m.named_parameters():
        ref = g[f"grad_n{n}/{k}"]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=2e-3, atol=3e-6 * max(1.0, np.abs(ref).max()), err_msg=k)
    assert int(sd["backbone.bn0.num_batches_tracked"]) == 1


@pytest.mark.parametrize("blend", [True, False])
@pytest.mark.parametrize("s", [64, 128])
def test_baseline_config3_fusion_train_step_golden(blend, s):
    """BASELINE configs[2] (`--images --preop --survival [--blend]`): one training step at 64^3 and at the BASELINE extent
    2 x 2 x 128^3 against the numbers recorded from the reference's own classes (fp32 CPU).  Outputs / losses at the north-star
    bar (1e-4).  Gradients against this golden only loosely: the reference's fp32 ReLU branches at near-zero pre-activations
    differ from any other fp32 evaluation; the strict gradient check is test_baseline_config3_fusion_gradients_fp64."""
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    g = load_golden(f"g3_fusion_s{s}.npz")
    tag = "blend" if blend else "plain"
    mm = _zero_dropout(_fusion(blend))
    mm.train()
    x = {"image": image_in(2, 2, s).to(DEV), "clinical": clin_in(2).to(DEV)}
    ev, du = (t.to(DEV) for t in labels(2))
    out = mm(x)
    if blend:
        gb = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion)
        loss, sel = gb.computeLoss(out, ev, du)
        np.testing.assert_allclose(gb.computeLossSurv(out, ev, du, reduceToHeads=True).detach().cpu().numpy(), g[f"{tag}/head_losses"], rtol=1e-4)
        assert abs(sel.item() - g[f"{tag}/selection_loss"][0]) < 1e-4 * abs(sel.item())
    else:
        loss = surv_criterion(CoxPH, out, ev, du, DEV)
    loss.backward()
    assert rel_err(out.detach().cpu().numpy(), g[f"{tag}/out"]) < 1e-4
    assert abs(loss.item() - g[f"{tag}/loss"][0]) < 1e-4 * abs(loss.item())
    params = dict(mm.named_parameters())
    gl2 = float(g[f"{tag}/grad_global_l2"][0])
    mine = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values() if p.grad is not None)))
    assert abs(mine - gl2) < 0.05 * gl2
    for k, l2 in zip(g[f"{tag}/grad_names"], g[f"{tag}/grad_l2"]):
        k = str(k)
        if np.isnan(l2):
            assert params[k].grad is None, k        # class_layers / MLP output_head never receive a gradient
        else:
            assert params[k].grad is not None, k
    # BN running statistics after the step + eval-mode forward (G4)
    sd = mm.state_dict()
    for k, v in zip(g[f"{tag}/running_names"], g[f"{tag}/running_chk"]):
        t = sd[str(k)].double()
        np.testing.assert_allclose([t.sum().item(), t.abs().sum().item()], v, rtol=1e-4, atol=1e-5)
    assert int(sd["image_model.model.backbone.norm5.num_batches_tracked"]) == 1
    mm.eval()
    with torch.no_grad():
        oe = mm(x)
    assert rel_err(oe.cpu().numpy(), g[f"{tag}/eval_out"]) < 1e-4


def _device_relu_masks(bb, x, cfg):
    """ReLU branch decisions of the last training forward of backbone module `bb` on input `x`, keyed like the oracle's taps."""
    from mmnn_sts_amd import _lib
    ent = bb._plans[(tuple(x.shape), x.device.index)]
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, s = x.shape[0], x.shape[2]

    def fetch(kind, b, l, shape):
        m = torch.empty(shape, dtype=torch.uint8, device=DEV)
        _lib.check(L.mmnn_densenet_relu_mask(ent["plan"], bb._flat.data_ptr(), ent["ws"].data_ptr(), kind, b, l, m.data_ptr(), st), "relu_mask")
        return m.cpu()

    masks = {"relu0": fetch(0, 0, 0, (n, cfg.init_features, s // 2, s // 2, s // 2))}
    dims, c = s // 4, cfg.init_features
    mid = cfg.bn_size * cfg.growth_rate
    for b, nl in enumerate(cfg.block_config):
        for l in range(nl):
            masks[f"b{b + 1}l{l + 1}r1"] = fetch(1, b, l, (n, c, dims, dims, dims))
            masks[f"b{b + 1}l{l + 1}r2"] = fetch(2, b, l, (n, mid, dims, dims, dims))
            c += cfg.growth_rate
        if b != len(cfg.block_config) - 1:
            masks[f"t{b + 1}"] = fetch(3, b, 0, (n, c, dims, dims, dims))
            c //= 2
            dims //= 2
    return masks


def _compare_all_grads(named_params, sd):
    gl2 = float(torch.sqrt(sum((v.grad ** 2).sum() for v in sd.values() if v.is_floating_point() and v.grad is not None)))
    bad, seen = [], 0
    for k, p in named_params:
        ref = sd[k].grad
        if ref is None:
            assert p.grad is None, k
            continue
        seen += 1
        err = float((p.grad.double().cpu() - ref).norm())
        tol = 1e-3 * float(ref.norm()) + 1e-5 * gl2
        if err > tol:
            bad.append((k, err, float(ref.norm())))
    assert not bad, (len(bad), gl2, bad[:8])
    return seen


@pytest.mark.parametrize("s", [64, 128])
def test_baseline_config3_fusion_gradients_fp64(s):
    """BASELINE configs[2] with --blend: every one of the 394 parameter gradients of the blended training step (64^3 and the
    BASELINE extent 2 x 2 x 128^3) against the fp64 oracle taking the device's ReLU branches."""
    from mmnn_sts_amd import _lib
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    n = 2
    mm = _zero_dropout(_fusion(True))
    mm.train()
    x = {"image": image_in(n, 2, s).to(DEV), "clinical": clin_in(n).to(DEV)}
    ev, du = labels(n)
    out = mm(x)
    gb = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion)
    loss, _ = gb.computeLoss(out, ev.to(DEV), du.to(DEV))
    loss.backward()
    cfg = R.DenseNetCfg()
    masks = _device_relu_masks(mm.image_model.model.backbone, x["image"], cfg)
    sch = R.multimodal_schema(cfg, N_CLIN, 2, 12)
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in synth_sd(sch, "fusion.").items()}
    o64 = R.multimodal_forward(sd, image_in(n, 2, s).double(), clin_in(n).double(), cfg, True, True, mlp_dropout=0.0, relu_masks=masks)
    b64 = R.Blender()
    l64, _ = b64.compute_loss(o64, ev, du)
    b64.weights = b64.weights.double()
    l64, _ = b64.compute_loss(o64, ev, du)
    l64.backward()
    assert rel_err(out.detach().cpu().numpy(), o64.detach().numpy()) < 1e-4
    assert abs(loss.item() - l64.item()) < 1e-4 * abs(l64.item())
    assert _compare_all_grads(mm.named_parameters(), sd) == 394   # 398 tensors - the 4 that never get a gradient


def test_baseline_config3_fusion_gradients_fp64_dropout(monkeypatch):
    """The blended training step with NOTHING zeroed, as main.py and bench.py run it: DenseNet121 with Dropout3d 0.2 in every dense
    layer, element dropout 0.2 on the image features, Dropout1d 0.2 in the clinical MLP.  The stream ids are recorded in call order
    (backbone, image features, the MLP's two stacks), the restated masks of all of them (tests/_util.py) and the device's ReLU branches
    are imposed on the fp64 oracle: risk scores and loss at 1e-4, all 394 gradients at the tolerance of the dropout-free test.
    N = 4 at 64^3; torch.manual_seed is chosen on the CPU (tests/_dropout_cases.py: FUSION_TORCH_SEED, kept true by
    tests/test_dropout_cpu.py) such that the MLP's batch norm over the live rows is well conditioned."""
    from mmnn_sts_amd import _lib, ops
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    from tests import _dropout_cases as D
    from tests._util import backbone_drop_masks, feat_drop_mask_ref
    n, s, p = 4, 64, 0.2
    mm = _fusion(True, dropout=p)
    mm.train()
    assert sum(1 for m in mm.modules() if m.__class__.__name__.startswith("Dropout") and m.p == p) == 58 + 1 + 6
    monkeypatch.setattr(ops, "_seed_counter", [0])
    torch.manual_seed(D.FUSION_TORCH_SEED)
    drawn, orig = [], ops.next_seed
    monkeypatch.setattr(ops, "next_seed", lambda: drawn.append(orig()) or drawn[-1])
    feats = {}
    hooks = [mm.image_model.register_forward_hook(lambda m, i, o: feats.__setitem__("image", o.detach().cpu())),
             mm.clinical_model.register_forward_hook(lambda m, i, o: feats.__setitem__("clinical", o.detach().cpu()))]
    x = {"image": image_in(n, 2, s).to(DEV), "clinical": clin_in(n).to(DEV)}
    ev, du = labels(n)
    out = mm(x)
    for h in hooks:
        h.remove()
    gb = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion)
    loss, _ = gb.computeLoss(out, ev.to(DEV), du.to(DEV))
    loss.backward()
    monkeypatch.setattr(ops, "next_seed", orig)
    assert drawn == D.fusion_seeds(D.FUSION_TORCH_SEED)
    cfg = R.DenseNetCfg()
    case = D.fusion_mlp_case(D.FUSION_TORCH_SEED, n, p)
    drop_masks = backbone_drop_masks(cfg, drawn[0], n, p)
    feat_mask = torch.from_numpy(feat_drop_mask_ref(drawn[1], n, 12, p)).double()
    mlp_masks = case.masks()
    # the masks as the device took them, where its outputs show them: dropped image features, dead MLP rows
    assert torch.equal(feats["image"] == 0, feat_mask == 0) and bool((feat_mask == 0).any())
    assert bool((feats["clinical"].abs().sum(dim=1) == 0)[mlp_masks[5] == 0].all()) and D.well_formed(case)
    assert all(bool((m == 0).any()) and bool((m != 0).any()) for m in drop_masks.values())
    bb = mm.image_model.model.backbone
    masks = _device_relu_masks(bb, x["image"], cfg)
    ent = bb._plans[(tuple(x["image"].shape), x["image"].device.index)]
    off = _lib.lib().mmnn_densenet_ws_offset(ent["plan"], b"idx", 0, 0)
    pool = ent["ws"][off:off + n * cfg.init_features * (s // 4) ** 3].view(torch.uint8).view(n, cfg.init_features, s // 4, s // 4, s // 4).cpu()
    sch = R.multimodal_schema(cfg, N_CLIN, 2, 12)
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in synth_sd(sch, "fusion.").items()}
    taps = {}
    o64 = R.multimodal_forward(sd, image_in(n, 2, s).double(), clin_in(n).double(), cfg, True, True, mlp_dropout=p, relu_masks=masks,
                               taps=taps, pool_taps=pool,       # the stem's max-pool winners too: see tests/test_backbone_gpu.py::_run_case
                               drop_masks=drop_masks, feat_drop_mask=feat_mask, mlp_drop_masks=mlp_masks,
                               mlp_relu_masks={5: feats["clinical"] > 0})
    b64 = R.Blender()
    l64, _ = b64.compute_loss(o64, ev, du)
    b64.weights = b64.weights.double()
    l64, _ = b64.compute_loss(o64, ev, du)
    l64.backward()
    assert float(taps["pool_gap"].max()) <= 1e-4 * float(taps["stem"].detach().abs().max())
    eo, el = rel_err(out.detach().cpu().numpy(), o64.detach().numpy()), abs(loss.item() - l64.item()) / abs(l64.item())
    print("seeds", [hex(v) for v in drawn], "risk scores rel err", eo, "loss rel err", el)
    assert eo < 1e-4
    assert el < 1e-4
    assert _compare_all_grads(mm.named_parameters(), sd) == 394


@pytest.mark.parametrize("s", [64, 128, 256])
def test_baseline_config5_gradcam_golden(s):
    """BASELINE configs[4] (`--inference --images --preop --survival`): Grad-CAM on one patient, up to the BASELINE extent
    1 x 2 x 256^3, against the reference's MultiModalGradCAM (risk scores, both attention maps, hooked activations / gradients)."""
    g = load_golden(f"g5_gradcam_s{s}.npz")
    mm = _fusion(False, dropout=0.2)
    mm.eval()
    cam = mm.add_gradcam("unused")
    x = {"image": image_in(1, 2, s).to(DEV), "clinical": clin_in(1).to(DEV)}
    preds, maps = cam(x)
    assert rel_err(preds.cpu().numpy(), g["preds"]) < 1e-4
    assert len(maps) == 2 and tuple(maps[0].shape) == (s, s, s)
    for i, m in enumerate(maps):
        m = m.cpu()
        np.testing.assert_allclose(m[:: s // 8, :: s // 8, :: s // 8].numpy(), g[f"map{i}_coarse"], rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(stat3(m), g[f"map{i}_stats"], rtol=2e-3, atol=1e-4)
    np.testing.assert_allclose(cam.features.cpu().numpy(), g["act_after"], rtol=2e-3, atol=1e-6 * np.abs(g["act_after"]).max())
    np.testing.assert_allclose(cam.grads.cpu().numpy(), g["last_grads"], rtol=2e-3, atol=1e-6 * np.abs(g["last_grads"]).max())


@pytest.mark.parametrize("s", [64, 128])
def test_baseline_config2_unimodal_train_step(s):
    """BASELINE configs[1] (`--images --survival`, modality t1): DenseNet121(in=1) full forward incl. class_layers ->
    surv_criterion(CoxPH) -> backward (reference main.py:451,460,466,469) at 64^3 and at the BASELINE extent 2 x 1 x 128^3:
    risk scores / loss / running statistics / eval forward against the reference-generated golden at 1e-4, and every one of the
    366 gradients against the fp64 oracle taking the device's ReLU branches."""
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.models.densenet import DenseNet121
    from mmnn_sts_amd.utils.utils import surv_criterion
    g = load_golden(f"g8_unimodal_in1_s{s}.npz")
    cfg = R.DenseNetCfg(in_channels=1)
    sch = R.densenet_schema(cfg)
    m = DenseNet121(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, dropout_prob=0.0)
    _load(m, sch, "densenet.").to(DEV)
    m.train()
    n = 2
    x = image_in(n, 1, s).to(DEV)
    ev, du = labels(n)
    y = m(x)
    loss = surv_criterion(CoxPH, y, ev.to(DEV), du.to(DEV), DEV)
    loss.backward()
    assert rel_err(y.detach().cpu().numpy(), g["out"]) < 1e-4
    assert abs(loss.item() - g["loss"][0]) < 1e-4 * abs(g["loss"][0])
    params = dict(m.named_parameters())
    mine = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values())))
    assert abs(mine - float(g["grad_global_l2"][0])) < 0.05 * float(g["grad_global_l2"][0])
    # downstream of every ReLU: exact to fp32 round-off.  The bias gradient is analytically 0 (the Cox loss is invariant to a
    # shift of the risk scores), so it is compared absolutely, on the scale of the weight gradient.
    wscale = float(np.abs(g["grad/class_layers.out.weight"]).max())
    for k in ("class_layers.out.weight", "class_layers.out.bias"):
        np.testing.assert_allclose(params[k].grad.cpu().numpy(), g[f"grad/{k}"], rtol=2e-3, atol=1e-5 * wscale)
    sd_dev = m.state_dict()
    for k, v in zip(g["running_names"], g["running_chk"]):
        t = sd_dev[str(k)].double()
        np.testing.assert_allclose([t.sum().item(), t.abs().sum().item()], v, rtol=1e-4, atol=1e-5)
    # strict: fp64 oracle with the device's ReLU branches
    masks = _device_relu_masks(m.backbone, x, cfg)
    sd = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in synth_sd(sch, "densenet.").items()}
    y64 = R.densenet_forward(sd, image_in(n, 1, s).double(), cfg, True, relu_masks=masks)
    l64 = R.surv_criterion(R.CoxPH, y64, ev, du)
    l64.backward()
    assert rel_err(y.detach().cpu().numpy(), y64.detach().numpy()) < 1e-4
    assert abs(loss.item() - l64.item()) < 1e-4 * abs(l64.item())
    assert _compare_all_grads(m.named_parameters(), sd) == 366
    m.eval()
    with torch.no_grad():
        assert rel_err(m(x).cpu().numpy(), g["eval_out"]) < 1e-4


def test_unimodal_densenet_forward_golden():
    """DenseNet121(in=2) backbone -> features -> class_layers, train and eval, against G2 at 64^3."""
    from mmnn_sts_amd.models.densenet import DenseNet121
    g = load_golden("g2_densenet_in2_s64.npz")
    cfg = R.DenseNetCfg(in_channels=2)
    m = DenseNet121(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.0)
    _load(m, R.densenet_schema(cfg), "densenet.").to(DEV)
    m.train()
    x = image_in(2, 2, 64).to(DEV)
    h = m.backbone(x)
    f = m.features(h)
    y = m.class_layers(f)
    assert rel_err(h.detach().cpu().numpy(), g["norm5"]) < 1e-4
    assert rel_err(f.detach().cpu().numpy(), g["features"]) < 1e-4
    assert rel_err(y.detach().cpu().numpy(), g["out"]) < 1e-4
    m.eval()
    with torch.no_grad():
        assert rel_err(m(x).cpu().numpy(), g["eval_out"]) < 1e-4


def test_dropout_semantics_and_accumulation():
    """Dropout3d drops whole (n, c) channels of the new features; gradients accumulate across backward calls like autograd."""
    from mmnn_sts_amd.models.densenet import DenseNet
    torch.manual_seed(3)
    m = DenseNet(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, block_config=(2, 2), dropout_prob=0.5).to(DEV)
    m.train()
    x = torch.randn(4, 1, 24, 24, 24, device=DEV)
    h = m.backbone(x)
    bb = m.backbone
    ent = bb._plans[(tuple(x.shape), x.device.index)]
    from mmnn_sts_amd import _lib
    off = _lib.lib().mmnn_densenet_ws_offset(ent["plan"], b"x", 0, 0)
    xb = ent["ws"][off:off + 4 * 4 * 128 * 216].view(torch.float32).view(4, 128, 216)
    new = xb[:, 64:]                                        # the 2 x 32 channels produced by the dense layers
    zero = (new.abs().amax(dim=2) == 0)
    frac = zero.float().mean().item()
    assert 0.3 < frac < 0.7, frac                           # ~ p = 0.5 of the (n, c) channels are dropped entirely
    h.sum().backward()
    g1 = bb.flat_grad.clone()
    h2 = m.backbone(x)
    h2.sum().backward()                                     # no zero_grad: accumulates
    assert bb.conv0.weight.grad.data_ptr() == bb.flat_grad.data_ptr()
    assert float((bb.flat_grad - g1).abs().max()) > 0
    m.zero_grad(set_to_none=True)
    assert bb.conv0.weight.grad is None
    h3 = m.backbone(x)
    h3.sum().backward()                                     # after zero_grad: overwritten, not accumulated; views re-attached
    assert bb.conv0.weight.grad.data_ptr() == bb.flat_grad.data_ptr()
    from mmnn_sts_amd.optim import FusedSGD
    opt = FusedSGD(m, lr=0.0)
    g3 = bb.flat_grad.clone()
    opt.zero_grad()                                         # cheap path: views stay attached, buffer marked stale
    m.backbone(x).sum().backward()
    assert float((bb.flat_grad.abs().sum() - g3.abs().sum()).abs()) < 0.5 * float(g3.abs().sum())   # same magnitude: not doubled


def test_cox_fractional_durations_not_truncated():
    """float32 durations (data/ImageDatasets.py:462) are the WEIGHTS in the reference's call order; they must reach
    the kernel un-truncated.  Values from the reference's own CoxPH / surv_criterion (G9)."""
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    g = load_golden("g9_classification.npz")
    for n in (4, 9):
        h = torch.from_numpy(synth.uniform(f"coxf/h{n}", (n, 2))).to(DEV)
        ev = torch.from_numpy((synth.uniform(f"coxf/e{n}", (n, 2)) > -0.3).astype(np.float32))
        ev[0] = 1
        du = torch.from_numpy((synth.uniform(f"coxf/d{n}", (n, 2)) * 0.5 + 0.5).astype(np.float32) * 30.0 + 0.25)
        assert abs(surv_criterion(CoxPH, h, ev.to(DEV), du.to(DEV), DEV).item() - g[f"coxf/n{n}"][0]) < 1e-5 * g[f"coxf/n{n}"][0]
        assert abs(CoxPH(h[:, 0], ev[:, 0].to(DEV), du[:, 0].to(DEV)).item() - g[f"coxf/n{n}/c0"][0]) < 1e-5 * g[f"coxf/n{n}/c0"][0]
        # intended order: fractional durations as the SORT KEY -- against the fp64 oracle
        ref = R.pycox_cox_ph_loss(h[:, 0].cpu().double(), du[:, 0].double(), ev[:, 0].double())
        assert abs(CoxPH(h[:, 0], ev[:, 0].to(DEV), du[:, 0].to(DEV), intended_order=True).item() - ref.item()) < 1e-5 * abs(ref.item())


def test_cox_edge_cases_vs_oracle():
    """Edges of the Cox kernel against the fp64 oracle: a batch above 1024 patients (sort scratch in global memory instead of LDS,
    csrc/tail.hip), a single patient, and a weight sum of zero (the reference's 0 / 0 = NaN must come through, not an exception)."""
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import CoxPH
    from mmnn_sts_amd.utils.utils import surv_criterion
    for n in (1, 1024, 1025, 1500):
        p = torch.from_numpy(synth.uniform(f"coxe/p{n}", (3, n, 2))).double().requires_grad_(True)
        ev = torch.from_numpy((synth.uniform(f"coxe/e{n}", (n, 2)) > -0.3).astype(np.int64))
        ev[0] = 1
        du = torch.from_numpy((1 + np.floor((synth.uniform(f"coxe/d{n}", (n, 2)) * .5 + .5) * 2998)).astype(np.int64))
        b = R.Blender()
        b.weights = torch.tensor([0.5, 0.3, 0.2], dtype=torch.float64)
        loss, _ = b.compute_loss(p, ev, du)
        loss.backward()
        pg = p.detach().float().to(DEV).requires_grad_(True)
        gb = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion)
        gb.weights = torch.tensor([0.5, 0.3, 0.2], device=DEV)
        lg, _ = gb.computeLoss(pg, ev.to(DEV), du.to(DEV))
        lg.backward()
        # n = 1: the loss is log(1 + eps) = 1e-7 (1.19e-7 in float32) and the gradient 0 -- absolute floors for that case
        assert abs(lg.item() - loss.item()) < 1e-4 * abs(loss.item()) + 1e-6, n
        assert np.abs(pg.grad.cpu().numpy() - p.grad.numpy()).max() < 1e-4 * np.abs(p.grad.numpy()).max() + 1e-7, n
    h = torch.tensor([.3, -.2, .1, .4])
    ref = R.CoxPH(h.double(), torch.tensor([1, 0, 1, 1]), torch.zeros(4, dtype=torch.int64))
    got = CoxPH(h.to(DEV), torch.tensor([1, 0, 1, 1], device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
    assert torch.isnan(ref) and torch.isnan(got)


@pytest.mark.parametrize("red", ["sum", "mean"])
def test_classification_bce_and_blender_golden(red):
    """BASELINE configs[0] loss path on the device: pos-weighted BCE-with-logits kernel, `criterion`, and the blender's
    classification branch (losses/GradientBlender.py:105-136,150-179) against the reference's numbers (G9)."""
    from mmnn_sts_amd.losses.GradientBlender import GradientBlender
    from mmnn_sts_amd.losses.losses import BCEWithLogitsLoss
    from mmnn_sts_amd.utils.utils import criterion
    from tests.test_oracle import _cls_inputs, _cls_update_inputs
    g = load_golden("g9_classification.npz")
    pw = torch.from_numpy(g["pos_weight"]).to(DEV)
    logits, targets = (t.to(DEV) for t in _cls_inputs())
    assert abs(criterion(BCEWithLogitsLoss(pos_weight=pw, reduction='sum'), logits[0], targets, DEV).item() - g["criterion_sum"][0]) < 2e-6 * g["criterion_sum"][0]
    bce = BCEWithLogitsLoss(pos_weight=pw, reduction='none')
    x = logits.clone().requires_grad_(True)
    gb = GradientBlender(bce, reduction=red, device=DEV)
    loss = gb.computeLoss(x, targets)
    loss.backward()
    assert abs(loss.item() - g[f"{red}/loss"][0]) < 2e-6 * g[f"{red}/loss"][0]
    np.testing.assert_allclose(x.grad.cpu().numpy(), g[f"{red}/grad"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(gb.computeLoss(logits, targets, reduceToHeads=True).cpu().numpy(), g[f"{red}/heads"], rtol=2e-6)
    np.testing.assert_allclose(gb.computeLoss(logits, targets, no_reduce=True).cpu().numpy(), g["no_reduce"], rtol=2e-6, atol=1e-7)
    gb = GradientBlender(bce, device=DEV)
    for it in range(3):
        gb.updateWeights(*(t.to(DEV) for t in _cls_update_inputs(it)))
        np.testing.assert_allclose(gb.weights.cpu().numpy(), g["upd_weights"][it], rtol=3e-4, atol=1e-6)
    assert len(gb.history) == 1
    # extreme logits: the stable softplus form must not overflow
    big = torch.tensor([[80.0, -80.0], [-100.0, 100.0]], device=DEV, requires_grad=True)
    l = BCEWithLogitsLoss(reduction='sum')(big, torch.tensor([[1.0, 0.0], [1.0, 0.0]], device=DEV))
    l.backward()
    assert torch.isfinite(l) and abs(l.item() - 200.0) < 1e-3 and torch.isfinite(big.grad).all()


def test_eval_mode_backward_raises_and_n1_training_rejected():
    from mmnn_sts_amd.models.densenet import DenseNet
    from mmnn_sts_amd.models.mlp import MLP
    m = DenseNet(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, block_config=(2, 2)).to(DEV)
    x = torch.randn(2, 1, 32, 32, 32, device=DEV)
    m.eval()
    y = m(x)                                                   # grad mode on, eval mode: forward works ...
    with pytest.raises(RuntimeError, match="eval-mode"):
        y.sum().backward()                                     # ... a backward must not silently skip the backbone
    with torch.no_grad():
        assert torch.isfinite(m(x)).all()
    mlp = MLP(N_CLIN, 2, 12).to(DEV).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        mlp(torch.randn(1, N_CLIN, device=DEV))


@pytest.mark.parametrize("dhw", [(96, 64, 70), (64, 96, 128)])
def test_gradcam_ragged_extents_vs_oracle(dhw):
    """`mmnn_gradcam` off the cubic golden extents: a non-cubic captured layer (6x4x4 / 4x6x8), an output width that is not a multiple of 4
    (70: the up-sampling kernel's scalar store path) and one that is (128: 16-byte stores), against the fp64 oracle's autograd Grad-CAM
    (utils/utils.py:293-344 restated: per-class backward, in-place cumulative weighting, min-max, F.interpolate trilinear)."""
    from mmnn_sts_amd.models.densenet import DenseNet
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    cfg = R.DenseNetCfg(in_channels=2, block_config=(2, 2, 2))
    sch = R.multimodal_schema(cfg, N_CLIN, 2, 12)
    img = DenseNet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, block_config=(2, 2, 2), dropout_prob=0.2)
    mm = MultiModalModel(img, [f"p{i}" for i in range(N_CLIN)], 2, 12, blend=False)
    _load(mm, sch, "fusion.")
    mm = mm.to(DEV).eval()
    image = torch.from_numpy(synth.uniform(f"gc/{dhw}", (1, 2) + dhw))
    clinical = clin_in(1)
    cam = mm.add_gradcam("unused")
    preds, maps = cam({"image": image.to(DEV), "clinical": clinical.to(DEV)})
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in synth_sd(sch, "fusion.").items()}
    ref_out, ref_maps, ref_small = R.multimodal_gradcam(sd64, image.double(), clinical.double(), cfg)
    assert rel_err(preds.cpu().numpy(), ref_out.numpy()) < 1e-4
    assert len(maps) == 2 and tuple(maps[0].shape) == dhw and tuple(cam.heat.shape) == (2,) + tuple(ref_small[0].shape)
    for i in range(2):
        np.testing.assert_allclose(cam.heat[i].cpu().numpy(), ref_small[i].numpy(), rtol=2e-3, atol=2e-4)       # normalised low-resolution map
        np.testing.assert_allclose(maps[i].cpu().numpy(), ref_maps[i].numpy(), rtol=2e-3, atol=3e-4)            # every up-sampled voxel
        assert float(maps[i].min()) >= -1e-6 and float(maps[i].max()) <= 1.0 + 1e-6
