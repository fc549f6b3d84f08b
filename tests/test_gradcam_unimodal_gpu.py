"""Grad-CAM of image-only models (utils.GradCAM, `mmnn_gradcam_unimodal`) against fp64 autograd on the oracle: the rules pinned in
INTEGRATION.md ("Grad-CAM of image-only models") -- last Conv3d of the encoder, target = sum / one / argmax of each sample's outputs,
alpha = voxel mean of d target / d A, ReLU of the weighted channel sum, per-sample min-max (all-equal -> 0), trilinear up-sampling."""
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from oracle import synth
from tests._util import rel_err, synth_sd
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- fp64 references ------------------------------------------------------------------------------------------------------------
def _target(out, label):
    if label is None:
        return out.sum(1)
    if label == "best":
        return out.gather(1, out.argmax(1, keepdim=True))[:, 0]
    return out[:, label]


def _cam_from(out, act, label, extent):
    """Grad-CAM from the autograd graph out(act): gradient, alpha, ReLU(weighted sum), per-sample min-max, trilinear."""
    (g,) = torch.autograd.grad(_target(out, label).sum(), act)       # samples are independent in eval mode
    alpha = g.mean(dim=(2, 3, 4), keepdim=True)
    m = F.relu((alpha * act).sum(1, keepdim=True))
    lo, hi = m.amin(dim=(2, 3, 4), keepdim=True), m.amax(dim=(2, 3, 4), keepdim=True)
    heat = torch.where(hi > lo, (m - lo) / torch.where(hi > lo, hi - lo, torch.ones_like(hi)), torch.zeros_like(m))
    maps = F.interpolate(heat, size=extent, mode="trilinear", align_corners=False)
    return out.detach(), act.detach(), g, heat.detach(), maps.detach()


def densenet_ref(sd, x, cfg, label):
    """R.densenet_forward in eval mode; only the last conv2's weight needs a gradient for taps['last_conv'] to sit in the graph."""
    nb, nl = len(cfg.block_config), cfg.block_config[-1]
    key = f"backbone.denseblock{nb}.denselayer{nl}.layers.conv2.weight"
    leaf = {k: (v.double().clone().requires_grad_(k == key) if v.is_floating_point() else v) for k, v in sd.items()}
    taps = {}
    out = R.densenet_forward(leaf, x.double(), cfg, False, taps=taps)
    return _cam_from(out, taps["last_conv"], label, tuple(x.shape[2:]))


def r3d_ref(sd, x, label):
    """Resnet18.forward in eval mode (models/resnet.py:152-167, as R.resnet18_forward) with the output of layer4's last conv2 -- before
    its BatchNorm -- as the captured layer."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}

    def bn(p, t):
        return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)

    with torch.no_grad():
        h = F.relu(bn("stem.1", F.conv3d(x.double(), sd["stem.0.weight"], None, stride=(1, 2, 2), padding=(1, 3, 3))))
    act = None
    for li, (planes, stride, nb) in enumerate(zip(R.R3D_PLANES, R.R3D_STRIDES, R.R3D_BLOCKS), start=1):
        for b in range(nb):
            p = f"layer{li}.{b}"
            s = stride if b == 0 else 1
            last = li == 4 and b == nb - 1
            with torch.set_grad_enabled(last):
                out = F.relu(bn(f"{p}.conv1.1", F.conv3d(h, sd[f"{p}.conv1.0.weight"], None, stride=s, padding=1)))
                y = F.conv3d(out, sd[f"{p}.conv2.0.weight"], None, stride=1, padding=1)
                if last:
                    act = y.detach().requires_grad_(True)
                    y = act
                res = h
                if f"{p}.downsample.0.weight" in sd:
                    res = bn(f"{p}.downsample.1", F.conv3d(h, sd[f"{p}.downsample.0.weight"], None, stride=s))
                h = F.relu(bn(f"{p}.conv2.1", y) + res)
    out = torch.sigmoid(F.linear(F.adaptive_avg_pool3d(h, 1).flatten(1), sd["fc.weight"], sd["fc.bias"]))
    return _cam_from(out, act, label, tuple(x.shape[2:]))


# ---- models -----------------------------------------------------------------------------------------------------------------------
def _densenet(cls, in_ch, block_config=None, prefix="gcu.", dropout=0.2):
    from mmnn_sts_amd.models import densenet as D
    kw = dict(spatial_dims=3, in_channels=in_ch, out_channels=2, feature_channels=12, dropout_prob=dropout)
    if block_config is not None:
        kw["block_config"] = block_config
    m = getattr(D, cls)(**kw)
    cfg = R.DenseNetCfg(in_channels=in_ch, block_config=tuple(m.backbone.cfg["block_config"]), dropout_prob=dropout)
    sd = synth_sd(R.densenet_schema(cfg), prefix)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), sd, cfg


def _r3d(prefix="gcu.r3d."):
    from mmnn_sts_amd.models.resnet import r3d_18
    m = r3d_18(2)
    sd = synth_sd(R.resnet18_schema(2), prefix)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), sd


def _image(n, c, dhw, tag):
    return torch.from_numpy(synth.uniform(f"gcu/{tag}/{n}x{c}x{dhw}", (n, c) + tuple(dhw)))


def _check(cam, preds, maps, ref, n, c_cap, dhw):
    out_r, act_r, g_r, heat_r, maps_r = (t.numpy() for t in ref)
    assert rel_err(preds.cpu().numpy(), out_r) < 1e-4
    assert tuple(maps.shape) == (n, 1) + tuple(dhw) and maps.dtype == torch.float32 and maps.is_cuda
    assert tuple(cam.features.shape) == (n, c_cap) + tuple(act_r.shape[2:]) and tuple(cam.heat.shape) == (n, 1) + tuple(act_r.shape[2:])
    assert rel_err(cam.features.cpu().numpy(), act_r) < 1e-4
    np.testing.assert_allclose(cam.heat.cpu().numpy(), heat_r, rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(maps.cpu().numpy(), maps_r, rtol=2e-3, atol=3e-4)
    np.testing.assert_allclose(cam.grads.cpu().numpy(), g_r, rtol=2e-3, atol=1e-6 * np.abs(g_r).max())
    assert float(maps.min()) >= 0.0 and float(maps.max()) <= 1.0 + 1e-6 and bool(torch.isfinite(maps).all())


# ---- DenseNet family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", [None, 0, 1, "best"])
def test_densenet_batch3_vs_oracle(label):
    from mmnn_sts_amd.utils.utils import GradCAM
    m, sd, cfg = _densenet("DenseNet", 2, (2, 2, 2))
    x = _image(3, 2, (64, 64, 64), "dn")
    cam = GradCAM(m, label=label)
    preds, maps = cam(x.to(DEV))
    assert cam.layer_name == "backbone.denseblock3.denselayer2.layers.conv2"
    _check(cam, preds, maps, densenet_ref(sd, x, cfg, label), 3, 32, (64, 64, 64))


def test_densenet_ragged_extent_vs_oracle():
    """(96, 64, 70): a non-cubic captured layer and an output width that is not a multiple of 4 (the up-sampler's scalar stores)."""
    from mmnn_sts_amd.utils.utils import add_gradcam
    m, sd, cfg = _densenet("DenseNet", 2, (2, 2, 2))
    x = _image(2, 2, (96, 64, 70), "dn-ragged")
    cam = add_gradcam(m, "unused", multimodal=False)
    preds, maps = cam(x.to(DEV))
    _check(cam, preds, maps, densenet_ref(sd, x, cfg, None), 2, 32, (96, 64, 70))


def test_tinydensenet_in1_vs_oracle():
    from mmnn_sts_amd.utils.utils import GradCAM
    m, sd, cfg = _densenet("TinyDensenet", 1)
    x = _image(1, 1, (64, 64, 64), "tiny")
    cam = GradCAM(m)
    preds, maps = cam(x.to(DEV))
    assert cam.layer_name == "backbone.denseblock3.denselayer4.layers.conv2"
    _check(cam, preds, maps, densenet_ref(sd, x, cfg, None), 1, 32, (64, 64, 64))


def test_densenet121_in1_baseline_extent_vs_oracle():
    """BASELINE configs[1]'s model and extent: DenseNet121, one channel, 2 x 1 x 128^3."""
    from mmnn_sts_amd.utils.utils import GradCAM
    m, sd, cfg = _densenet("DenseNet121", 1)
    x = _image(2, 1, (128, 128, 128), "dn121")
    cam = GradCAM(m, label="best")
    preds, maps = cam(x.to(DEV))
    assert cam.layer_name == "backbone.denseblock4.denselayer16.layers.conv2"
    _check(cam, preds, maps, densenet_ref(sd, x, cfg, "best"), 2, 32, (128, 128, 128))


# ---- r3d_18 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dhw,label", [((32, 64, 64), None), ((64, 64, 64), "best"), ((64, 64, 64), 0)])
def test_r3d18_vs_oracle(dhw, label):
    from mmnn_sts_amd.utils.utils import GradCAM
    m, sd = _r3d()
    x = _image(2, 1, dhw, "r3d")
    cam = GradCAM(m, label=label)
    preds, maps = cam(x.to(DEV))
    assert cam.layer_name == "layer4.1.conv2.0"
    _check(cam, preds, maps, r3d_ref(sd, x, label), 2, 16, dhw)


# ---- properties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["densenet", "r3d"])
def test_samples_are_independent(kind):
    from mmnn_sts_amd.utils.utils import GradCAM
    m = _densenet("DenseNet", 1, (2, 2, 2))[0] if kind == "densenet" else _r3d()[0]
    x = _image(4, 1, (64, 64, 64), f"indep-{kind}").to(DEV)
    cam = GradCAM(m, label="best")
    _, maps = cam(x)
    maps = maps.clone()
    for b in range(4):
        _, one = cam(x[b:b + 1].contiguous())
        assert float((one[0] - maps[b]).abs().max()) <= 1e-6, b


@pytest.mark.parametrize("kind", ["densenet", "r3d"])
def test_zero_map_rule(kind):
    """All-zero weights after the captured layer: every gradient is 0, so is every map -- exactly, without NaN."""
    from mmnn_sts_amd.utils.utils import GradCAM
    if kind == "densenet":
        m = _densenet("DenseNet", 2, (2, 2, 2))[0]
        m.class_layers.out.weight.data.zero_()
        x = _image(2, 2, (64, 64, 64), "zero")
    else:
        m = _r3d()[0]
        m.fc.weight.data.zero_()
        x = _image(2, 1, (32, 64, 64), "zero")
    cam = GradCAM(m)
    _, maps = cam(x.to(DEV))
    assert bool(torch.isfinite(maps).all()) and bool(torch.isfinite(cam.heat).all())
    assert float(maps.abs().max()) == 0.0 and float(cam.heat.abs().max()) == 0.0 and float(cam.grads.abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["densenet", "r3d"])
def test_repeated_calls_are_bit_identical(kind):
    from mmnn_sts_amd.utils.utils import GradCAM
    m = _densenet("DenseNet", 2, (2, 2, 2))[0] if kind == "densenet" else _r3d()[0]
    x = _image(3, 2 if kind == "densenet" else 1, (64, 48, 40), f"rep-{kind}").to(DEV)
    cam = GradCAM(m)
    first = [t.clone() for t in cam(x)] + [cam.heat.clone(), cam.grads.clone()]
    for _ in range(2):
        again = list(cam(x)) + [cam.heat, cam.grads]
        assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("kind", ["densenet", "r3d"])
def test_outputs_match_eval_forward_and_training_is_unaffected(kind):
    """`outputs` is the model's own eval forward, bit for bit; the wrapper leaves every module's mode, the running statistics and a
    following training forward as they were."""
    from mmnn_sts_amd.utils.utils import GradCAM
    if kind == "densenet":
        m = _densenet("DenseNet", 2, (2, 2, 2), dropout=0.0)[0]
        x = _image(2, 2, (64, 64, 64), "io").to(DEV)
    else:
        m = _r3d()[0]
        m.dropout.p = 0.0
        x = _image(2, 1, (32, 64, 64), "io").to(DEV)
    twin = copy.deepcopy(m)
    with torch.no_grad():
        ref = m.eval()(x)
    m.train()
    next(iter(m.children())).eval()                       # a mixed state must come back as it was
    modes = [mod.training for mod in m.modules()]
    running = lambda: [t.clone() for name, t in m.named_buffers() if "running" in name]
    stats = running()
    preds, _ = GradCAM(m)(x)
    assert torch.equal(preds, ref)
    assert [mod.training for mod in m.modules()] == modes
    assert all(torch.equal(a, b) for a, b in zip(stats, running()))
    m.train()
    twin.train()
    torch.testing.assert_close(m(x), twin(x), rtol=1e-6, atol=1e-7)


def test_label_out_of_range_is_an_error():
    from mmnn_sts_amd.utils.utils import GradCAM
    m = _densenet("DenseNet", 2, (2, 2, 2))[0]
    with pytest.raises(ValueError, match="label"):
        GradCAM(m, label=2)(_image(1, 2, (32, 32, 32), "lbl").to(DEV))


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------
_run = functools.partial(run_main, limit_s=900)


def test_cli_inference_images_survival_writes_maps(tmp_path):
    """`--inference --images --survival` of a one-channel TinyDensenet (BASELINE configs[1]'s model) writes one (D, H, W) map per
    patient; `--no_gradcam` writes none."""
    from mmnn_sts_amd.models.densenet import TinyDensenet
    cfg = tiny_config(tmp_path, "t1", 1)
    torch.manual_seed(3)
    weights = tmp_path / "model.pth"
    torch.save(TinyDensenet(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, dropout_prob=0.2).state_dict(), weights)
    common = ["--inference", "--images", "--survival", "--weights", str(weights), "--synthetic_patients", "8", "--synthetic_size", "32",
              "--config", cfg]
    with_maps = tmp_path / "maps"
    with_maps.mkdir()
    log = _run(common, with_maps)
    assert "All C-indexes" in log
    files = sorted(p.name for p in (with_maps / "attention_maps").iterdir())
    assert files == ["patient0_att_map.npy", "patient1_att_map.npy"]
    for f in files:
        a = np.load(with_maps / "attention_maps" / f)
        assert a.shape == (32, 32, 32) and a.dtype == np.float32
        assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0 + 1e-6
    without = tmp_path / "nomaps"
    without.mkdir()
    _run(common + ["--no_gradcam"], without)
    assert not list((without / "attention_maps").glob("*.npy"))
