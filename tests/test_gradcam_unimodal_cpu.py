"""`not gpu` side of the image-only Grad-CAM: add_gradcam(model, multimodal=False) builds for every supported encoder without a GPU
and names the captured layer (the last Conv3d in module-registration order); other models and labels are refused; the C-ABI entry
validates its descriptor on the host, before any launch."""
import ctypes
import os

import pytest
import torch.nn as nn


@pytest.fixture(scope="module")
def lib():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def _dn(cls, **kw):
    from mmnn_sts_amd.models import densenet as D
    return getattr(D, cls)(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, **kw)


@pytest.mark.parametrize("make,layer", [
    (lambda: _dn("DenseNet", block_config=(2, 2, 2)), "backbone.denseblock3.denselayer2.layers.conv2"),
    (lambda: _dn("TinyDensenet"), "backbone.denseblock3.denselayer4.layers.conv2"),
    (lambda: _dn("DenseNet121"), "backbone.denseblock4.denselayer16.layers.conv2"),
    (lambda: __import__("mmnn_sts_amd.models.resnet", fromlist=["r3d_18"]).r3d_18(2), "layer4.1.conv2.0"),
])
def test_add_gradcam_names_the_last_conv3d(make, layer):
    from mmnn_sts_amd.utils.utils import GradCAM, add_gradcam
    model = make()
    cam = add_gradcam(model, "attention_maps", multimodal=False)
    assert isinstance(cam, GradCAM) and cam.model is model and cam.label is None
    assert cam.layer_name == layer
    assert [n for n, m in model.named_modules() if isinstance(m, nn.Conv3d)][-1] == layer
    assert isinstance(model.get_submodule(layer), nn.Conv3d)
    assert cam.features is None and cam.grads is None and cam.heat is None


@pytest.mark.parametrize("make", [
    lambda: __import__("mmnn_sts_amd.models.mlp", fromlist=["MLP"]).MLP(32, 2, 12),
    lambda: nn.Sequential(nn.Conv3d(1, 4, 3), nn.ReLU()),
])
def test_unsupported_model_raises_type_error(make):
    from mmnn_sts_amd.utils.utils import add_gradcam
    with pytest.raises(TypeError, match="DenseNet121, TinyDensenet"):
        add_gradcam(make(), multimodal=False)


@pytest.mark.parametrize("label", [-1, 1.5, "worst", True])
def test_bad_label_is_refused(label):
    from mmnn_sts_amd.utils.utils import GradCAM
    with pytest.raises(ValueError, match="label"):
        GradCAM(_dn("DenseNet", block_config=(2, 2, 2)), label=label)


def test_c_abi_validates_before_launching(lib):
    from mmnn_sts_amd import _lib
    d = _lib.GradcamUnimodalDesc(4, 16, 16, 8, 8, 128, 128, 128, 2, _lib.GC_LABEL_BEST, 16 * 1024, 16 * 1024)
    ws = lib.mmnn_gradcam_unimodal_workspace_bytes(ctypes.byref(d))
    assert ws >= 4 * (4 * 16 + 4 * 1 * 16 + 4 * 1 * 2)
    bad = _lib.GradcamUnimodalDesc(4, 16, 0, 8, 8, 128, 128, 128, 2, -1, 0, 0)
    assert lib.mmnn_gradcam_unimodal_workspace_bytes(ctypes.byref(bad)) == -1
    fake = 256                                     # never dereferenced: every check below fails before the first launch
    head = _lib.GradcamHead(_lib.GC_HEAD_SIGMOID, 0, 0, 0, fake, None, fake, fake, fake, 1e-5)

    def call(desc, ws_bytes=ws):
        return lib.mmnn_gradcam_unimodal(ctypes.byref(desc), ctypes.byref(head), fake, fake, None, fake, fake, fake, ws_bytes, None)

    for field, value, text in (("label", 2, "label 2"), ("channels", 65, "width 65"), ("act_ns", 100, "sample stride"),
                               ("n", 0, "samples")):
        e = _lib.GradcamUnimodalDesc.from_buffer_copy(d)
        setattr(e, field, value)
        assert call(e) == 1 and text in _lib.last_error()
    assert call(d, ws - 1) == 1 and "workspace" in _lib.last_error()
    head.kind = 7
    assert call(d) == 1 and "head kind 7" in _lib.last_error()
