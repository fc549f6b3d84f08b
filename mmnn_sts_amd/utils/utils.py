"""Mirror of the helpers of utils/utils.py (DigITs-AIML/MMNN_STS) that sit on the fusion training path.

Kept (same names / signatures): `criterion` (:20-22), `surv_criterion` (:24-29), `save_model` (:31-35),
`BackpropagatableFeatureExtractor` (:238-251), `MultiModalGradCAM` (:253-344), `loadWeights` (:357-390, local files),
`add_gradcam` (:451-455), `loadUIDs` (:175-181, local files).  S3 / matplotlib helpers are host-side I/O outside the hot path
 and are not reproduced.  In place of the third-party `medcam.inject(backend='gcam')` that upstream's
`add_gradcam(model, multimodal=False)` returns, `GradCAM` computes the published Grad-CAM on the HIP path.
"""
import logging
import os

import torch
import torch.nn as nn

from .. import _lib, ops

logger = logging.getLogger(__name__)


def criterion(loss_func, preds, labels, device):
    return loss_func(preds, labels).to(device)


def surv_criterion(loss_func, preds, events, durations, device):
    """Sum of the survival loss over the C target columns (utils/utils.py:24-29).  With the package's `CoxPH` on the GPU all
    columns are evaluated by one kernel; any other callable is applied column by column like the reference does."""
    from ..losses import losses as _l
    if loss_func is _l.CoxPH and preds.is_cuda and preds.dim() == 2:
        loss, _ = ops.CoxBlend.apply(preds.unsqueeze(0), events, durations, None)
        return loss
    total = 0
    for i in range(preds.shape[1]):
        total = total + loss_func(preds[:, i], events[:, i], durations[:, i]).to(device)
    return total


def save_model(model, model_dir):
    logger.info("Saving the model.")
    torch.save(model.cpu().state_dict(), os.path.join(model_dir, 'model.pth'))


def loadUIDs(path):
    with open(path) as f:
        return [int(line.strip()) for line in f.readlines()]


class BackpropagatableFeatureExtractor(nn.Module):
    """`features(backbone(x))`, skipping the wrapped model's own classifier (utils/utils.py:238-251)."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model.features(self.model.backbone(x))


class MultiModalGradCAM(nn.Module):
    """Grad-CAM of the fusion model on the LAST Conv3d of the image backbone (= last dense layer's conv2), reproducing
    utils/utils.py:253-344 including its quirks: batch size 1 only (:334), channel-pooled gradients weight the activations
    IN PLACE and CUMULATIVELY across classes (:313-314), min-max normalisation, trilinear up-sampling to the input size.

    The reference runs a full autograd backward per class and keeps only d out[0,cls] / d act.  Here the eval-mode forward is the
    HIP backbone and everything after it is ONE C-ABI call (`mmnn_gradcam`, csrc/gradcam.hip): that single gradient in closed form
    (head -> feature_layer -> GAP -> ReLU mask -> norm5 scale, restricted to the last `growth_rate` channels; no weight gradients),
    the pooled weighting, the channel mean, the min-max normalisation and the trilinear up-sampling.  torch allocates the outputs.
    """

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.input_shape = None
        self.features = None
        self.grads = None

    def forward(self, x):
        import ctypes
        mm = self.model
        if getattr(mm, "blend", False):
            raise ValueError("MultiModalGradCAM expects blend=False (a (N, C) output), as main.py's inference path uses it")
        dn = mm.image_model.model
        bb = dn.backbone
        was_training = mm.training
        mm.eval()
        with torch.no_grad():
            image = x['image']
            assert image.shape[0] == 1, 'Batch dimension found in attention map - Must use batch size 1 when computing attention maps'
            h = bb(image)                                           # norm5 output, eval statistics
            ent = bb._plans[(tuple(image.shape), image.device.index)]
            L = _lib.lib()
            nb = len(bb.cfg["block_config"]) - 1
            ctot, g = h.shape[1], bb.cfg["growth_rate"]
            sp = tuple(h.shape[2:])
            v = h[0, 0].numel()
            # output of the last conv2 (dropout is off in eval) = the last `g` channels of the last block's concat buffer
            act_in = ent["ws"].data_ptr() + L.mmnn_densenet_ws_offset(ent["plan"], b"x", nb, 0) + 4 * (ctot - g) * v
            fi = dn.features(h)
            fc = mm.clinical_model(x['clinical'])
            outputs = ops.FusionHeads.apply(fi, fc, mm.output_head.weight, mm.output_head.bias, mm.image_output_head.weight,
                                            mm.image_output_head.bias, mm.clinical_output_head.weight, mm.clinical_output_head.bias, False)
            n5, wfeat, whead = bb.norm5, dn.features.feature_layer.weight, mm.output_head.weight
            ncls = outputs.shape[1]
            dev = h.device
            self.input_shape = image.shape
            D, H, W = (int(t) for t in image.shape[2:])
            act = torch.empty((1, g) + sp, device=dev, dtype=torch.float32)
            grads = torch.empty((1, g) + sp, device=dev, dtype=torch.float32)
            heat = torch.empty((ncls,) + sp, device=dev, dtype=torch.float32)
            maps = torch.empty((ncls, D, H, W), device=dev, dtype=torch.float32)
            desc = _lib.GradcamDesc(ctot, g, sp[0], sp[1], sp[2], ncls, wfeat.shape[0], whead.shape[1], D, H, W, float(n5.eps))
            for t in (h, wfeat, whead, n5.weight, n5.running_var):
                if not (t.is_contiguous() and t.dtype == torch.float32):
                    raise RuntimeError("MultiModalGradCAM expects contiguous float32 model tensors")
            _lib.enqueue("mmnn_gradcam", ctypes.byref(desc), h.data_ptr(), act_in, whead.data_ptr(), wfeat.data_ptr(), n5.weight.data_ptr(),
                         n5.running_var.data_ptr(), act.data_ptr(), grads.data_ptr(), heat.data_ptr(), maps.data_ptr())
            assert heat.ndim == 4, 'Batch dimension found in attention map - Must use batch size 1 when computing attention maps'
            att_maps = list(maps.unbind(0))
            self.features, self.grads, self.heat = act, grads, heat
        mm.train(was_training)
        return outputs, att_maps


class GradCAM(nn.Module):
    """Grad-CAM (Selvaraju et al.) of an image-only model -- DenseNet / DenseNet121 / TinyDensenet or r3d_18 -- on the last Conv3d of
    its encoder in module-registration order, for a whole batch: what upstream obtains from medcam's `gcam` backend
    (utils/utils.py:451-455).  Rules, and where they part from medcam, are pinned in INTEGRATION.md ("Grad-CAM of image-only models").

    `label`: None targets the sum of each sample's outputs, an int k output k, "best" the argmax of each sample's outputs (chosen on the
    device).  `cam(x)` returns `(outputs, att_maps)`: the outputs of `model.eval()(x)` and a (B, 1, D, H, W) fp32 tensor of per-sample
    min-max normalised maps in [0, 1] (an all-equal map is all zeros).  Afterwards `.features` holds the captured activations A
    (B, C, d, h, w; for a DenseNet a view into the backbone's workspace, valid until its next forward of that input shape), `.grads`
    d target / d A, `.heat` the (B, 1, d, h, w) normalised low-resolution maps and `.layer_name` the captured module.

    The eval forward is the model's own HIP path (for r3d_18 the wrapper runs the last BasicBlock itself with the same ops, to keep
    the pre-BN convolution output); everything after it is ONE C-ABI call (`mmnn_gradcam_unimodal`, csrc/gradcam_unimodal.hip):
    the gradient in closed form, the channel weights, ReLU, normalisation and up-sampling.  torch only allocates.
    """

    SUPPORTED = "DenseNet, DenseNet121, TinyDensenet (mmnn_sts_amd.models.densenet) and r3d_18 (mmnn_sts_amd.models.resnet.Resnet18)"

    def __init__(self, model, label=None):
        super().__init__()
        from ..models.densenet import DenseNet
        from ..models.resnet import BasicBlock, Resnet18
        if isinstance(model, DenseNet):
            kind = "densenet"
            nb = len(model.backbone.cfg["block_config"])
            expected = f"backbone.denseblock{nb}.denselayer{model.backbone.cfg['block_config'][-1]}.layers.conv2"
        elif isinstance(model, Resnet18) and isinstance(model.layer4[-1], BasicBlock):
            kind = "r3d_18"
            expected = f"layer4.{len(model.layer4) - 1}.conv2.0"
        else:
            raise TypeError(f"GradCAM supports {self.SUPPORTED}; got {type(model).__name__}")
        if not (label is None or label == "best" or (isinstance(label, int) and not isinstance(label, bool) and label >= 0)):
            raise ValueError(f"GradCAM label must be None, a non-negative int or 'best', got {label!r}")
        convs = [name for name, m in model.named_modules() if isinstance(m, nn.Conv3d)]
        if not convs or convs[-1] != expected:
            raise TypeError(f"GradCAM: the last Conv3d of this {type(model).__name__} is {convs[-1] if convs else None}, "
                            f"the closed-form gradient assumes {expected}")
        self.model = model
        self.kind = kind
        self.label = label
        self.layer_name = expected
        self.features = None
        self.grads = None
        self.heat = None

    def _label_code(self):
        if self.label is None:
            return _lib.GC_LABEL_SUM
        if self.label == "best":
            return _lib.GC_LABEL_BEST
        return int(self.label)

    def _densenet(self, x):
        m = self.model
        bb = m.backbone
        h = bb(x)                                                   # norm5 output (eval statistics)
        outputs = m.class_layers(m.features(h))                     # = DenseNet.forward
        ent = bb._plans[(tuple(x.shape), x.device.index)]
        L = _lib.lib()
        n, ctot = h.shape[0], h.shape[1]
        g = bb.cfg["growth_rate"]
        sp = tuple(h.shape[2:])
        v = h[0, 0].numel()
        # the last dense block's concat buffer is [N][c_total][v] (csrc/densenet.hip: the `concat` view, sample stride c_total * v); its last `g`
        # channels are the output of the last conv2 (dropout is the identity in eval)
        off = L.mmnn_densenet_ws_offset(ent["plan"], b"x", len(bb.cfg["block_config"]) - 1, 0)
        if off < 0:
            raise RuntimeError("GradCAM: no concat buffer in the DenseNet plan")
        buf = ent["ws"][off:off + 4 * n * ctot * v].view(torch.float32).view((n, ctot) + sp)
        act = buf[:, ctot - g:]
        n5, wfeat, wout = bb.norm5, m.features.feature_layer.weight, m.class_layers.out.weight
        for t in (h, wfeat, wout, n5.weight, n5.running_var):
            if not (t.is_contiguous() and t.dtype == torch.float32):
                raise RuntimeError("GradCAM expects contiguous float32 model tensors")
        head = _lib.GradcamHead(_lib.GC_HEAD_DENSENET, wfeat.shape[0], wfeat.shape[1], ctot - g, wout.data_ptr(), wfeat.data_ptr(),
                                n5.weight.data_ptr(), n5.running_var.data_ptr(), outputs.data_ptr(), float(n5.eps))
        mask = h[:, ctot - g:]
        return outputs, act, mask, ctot * v, ctot * v, head

    def _r3d(self, x):
        from ..models.resnet import _bn, _conv
        m = self.model
        if not x.is_cuda:
            raise RuntimeError("mmnn_sts_amd: r3d_18 runs on the MI355X only (no CPU path); move model and input to cuda")
        if x.dim() != 5 or x.shape[1] != m.stem[0].in_channels:
            raise ValueError(f"expected (N, {m.stem[0].in_channels}, D, H, W) input, got {tuple(x.shape)}")
        h = m.stem(x)                                               # = Resnet18.forward in eval mode (no dropout) ...
        for stage in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in stage:
                if blk is not m.layer4[-1]:
                    h = blk(h, drop_p=0.0)
        last = m.layer4[-1]                                         # ... with BasicBlock.forward of the last block unrolled
        out = _bn(_conv(h, last.conv1[0]), last.conv1[1], relu=True)
        act = _conv(out, last.conv2[0])                             # the captured layer, before its BatchNorm
        residual = h if last.downsample is None else _bn(_conv(h, last.downsample[0]), last.downsample[1], relu=False)
        y = _bn(act, last.conv2[1], relu=True, residual=residual)
        outputs = ops.GapFcSigmoid.apply(y, m.fc.weight, m.fc.bias)
        bn, wfc = last.conv2[1], m.fc.weight
        for t in (act, y, wfc, bn.weight, bn.running_var, outputs):
            if not (t.is_contiguous() and t.dtype == torch.float32):
                raise RuntimeError("GradCAM expects contiguous float32 model tensors")
        head = _lib.GradcamHead(_lib.GC_HEAD_SIGMOID, 0, 0, 0, wfc.data_ptr(), None, bn.weight.data_ptr(), bn.running_var.data_ptr(),
                                outputs.data_ptr(), float(bn.eps))
        c, v = act.shape[1], act[0, 0].numel()
        return outputs, act, y, c * v, c * v, head

    def _attention(self, captured, extent):
        """Everything after the encoder forward: ONE C-ABI call on the captured tensors.  Returns the (B, 1, D, H, W) maps and sets
        .features / .grads / .heat."""
        import ctypes
        outputs, act, mask, act_ns, mask_ns, head = captured
        n, c = act.shape[0], act.shape[1]
        sp = tuple(act.shape[2:])
        D, H, W = (int(t) for t in extent)
        dev = act.device
        desc = _lib.GradcamUnimodalDesc(n, c, sp[0], sp[1], sp[2], D, H, W, outputs.shape[1], self._label_code(), act_ns, mask_ns)
        ws_bytes = _lib.lib().mmnn_gradcam_unimodal_workspace_bytes(ctypes.byref(desc))
        if ws_bytes < 0:
            raise ValueError(f"GradCAM: bad captured layer {tuple(act.shape)}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        grads = torch.empty((n, c) + sp, device=dev, dtype=torch.float32)
        heat = torch.empty((n, 1) + sp, device=dev, dtype=torch.float32)
        maps = torch.empty((n, 1, D, H, W), device=dev, dtype=torch.float32)
        _lib.enqueue("mmnn_gradcam_unimodal", ctypes.byref(desc), ctypes.byref(head), act.data_ptr(), mask.data_ptr(), grads.data_ptr(),
                     heat.data_ptr(), maps.data_ptr(), ws.data_ptr(), ws_bytes)
        self.features, self.grads, self.heat = act, grads, heat
        return maps

    def forward(self, x):
        m = self.model
        modes = [(mod, mod.training) for mod in m.modules()]
        m.eval()
        try:
            with torch.no_grad():
                captured = self._densenet(x) if self.kind == "densenet" else self._r3d(x)
                maps = self._attention(captured, x.shape[2:])
        finally:
            for mod, mode in modes:
                mod.training = mode
        return captured[0], maps


def add_gradcam(model, output_dir='attention_maps', multimodal=False):
    """utils/utils.py:451-455.  multimodal: the fusion model's MultiModalGradCAM; otherwise `GradCAM` over the image-only model in place
    of upstream's medcam.inject(model, backend='gcam', return_attention=True) (parity unpinned against medcam)."""
    if multimodal:
        return model.add_gradcam(output_dir)
    return GradCAM(model)


def _occlusion_triple(name, v):
    """An int or a 3-sequence of ints >= 1 -> (d, h, w)."""
    t = tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3
    if len(t) != 3 or any(isinstance(e, bool) or not isinstance(e, int) or e < 1 for e in t):
        raise ValueError(f"OcclusionSensitivity: {name} must be a positive int or three of them (d, h, w), got {v!r}")
    return t


class OcclusionSensitivity(nn.Module):
    """Occlusion sensitivity maps: a `window` box of the input is replaced by `fill`, the model run, and the move of every output
    recorded; the box slides over the volume with `stride` and each voxel gets the mean move over the boxes that cover it.  The window
    grid, the fp64 summation order and the padding of the last batch are the contract above `mmnn_occlusion_window_count` in
    include/mmnn_sts.h (the last window of an axis is clamped to the edge, so every voxel is covered).

    `window`, `stride`: an int or (d, h, w), 1 <= stride <= window; `batch`: occluded samples per forward; `fill`: "mean" (the
    per-channel mean of the input it is given, computed on the device) or a float.  `occ(x)` takes a batch-1 input -- a (1, C, D, H, W)
    tensor or, with `multimodal`, the fusion model's {"image", "clinical"} dict, whose clinical row is repeated per occluded sample
    while only the image is occluded -- and returns `(outputs, maps)`: `outputs` is what `model.eval()(x)` returns, `maps` a
    (K, D, H, W) fp32 device tensor of RAW SIGNED deltas, one map per output: positive where hiding the region lowers that output.
    They are not min-max normalised: the sign and the scale are the information.

    Only the model's eval-mode forward is used, on its existing HIP path and under `torch.no_grad()`, so the supported models are
    exactly those whose own `eval()` forward supports a batch of `batch` samples (the fusion model with blend off, the image-only
    DenseNets, r3d_18); the model must return an (N, K) fp32 tensor with K <= 16.  The occluded batches (`mmnn_occlude_windows`), the
    fill (`mmnn_channel_means`) and the map (`mmnn_occlusion_map`) are HIP kernels (csrc/occlusion.hip); torch allocates and copies
    rows into the score table and does no arithmetic.  Parity with MONAI's OcclusionSensitivity is unpinned.
    """

    def __init__(self, model, window=16, stride=8, batch=8, fill="mean", multimodal=False):
        super().__init__()
        self.window = _occlusion_triple("window", window)
        self.stride = _occlusion_triple("stride", stride)
        for r, (w, s) in enumerate(zip(self.window, self.stride)):
            if s > w:
                raise ValueError(f"OcclusionSensitivity: stride {s} exceeds window {w} on axis {r}: voxels between the windows would never be hidden")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"OcclusionSensitivity: batch must be a positive int, got {batch!r}")
        if fill != "mean":
            if isinstance(fill, (bool, str)) or not isinstance(fill, (int, float)) or fill != fill or fill in (float("inf"), float("-inf")):
                raise ValueError(f"OcclusionSensitivity: fill must be 'mean' or a finite float, got {fill!r}")
            fill = float(fill)
        self.model = model
        self.batch = batch
        self.fill = fill
        self.multimodal = bool(multimodal)

    def _check_input(self, x):
        if self.multimodal:
            if not (isinstance(x, dict) and "image" in x and "clinical" in x):
                raise ValueError("OcclusionSensitivity(multimodal=True) expects the fusion model's {'image', 'clinical'} dict")
            if getattr(self.model, "blend", False):
                raise ValueError("OcclusionSensitivity expects blend=False (an (N, K) output), as main.py's inference path uses it")
            image = x["image"]
        else:
            image = x
        if not (torch.is_tensor(image) and image.dim() == 5 and image.shape[0] == 1):
            raise ValueError(f"OcclusionSensitivity takes one patient at a time: a (1, C, D, H, W) image, got "
                             f"{tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
        if not image.is_cuda:
            raise RuntimeError("mmnn_sts_amd: occlusion sensitivity runs on the MI355X only (no CPU path); move model and input to cuda")
        extent = tuple(int(t) for t in image.shape[2:])
        if any(w > e for w, e in zip(self.window, extent)):
            raise ValueError(f"OcclusionSensitivity: window {self.window} is larger than the input extent {extent}")
        return image.contiguous().float()

    def forward(self, x):
        import ctypes
        image = self._check_input(x)
        m = self.model
        modes = [(mod, mod.training) for mod in m.modules()]
        m.eval()
        try:
            with torch.no_grad():
                dev = image.device
                c, (d, h, w) = int(image.shape[1]), (int(t) for t in image.shape[2:])
                desc = _lib.OcclusionDesc(c, d, h, w, (ctypes.c_int32 * 3)(*self.window), (ctypes.c_int32 * 3)(*self.stride))
                wn = _lib.lib().mmnn_occlusion_window_count(ctypes.byref(desc), None)
                if wn < 0:
                    raise ValueError(f"OcclusionSensitivity: {_lib.last_error()}")
                outputs = m(dict(x, image=image) if self.multimodal else image)
                if not (outputs.dim() == 2 and outputs.shape[0] == 1 and outputs.dtype == torch.float32
                        and 1 <= outputs.shape[1] <= _lib.OCCLUSION_MAX_OUTPUTS):
                    raise ValueError(f"OcclusionSensitivity: the model must return a (1, K) float32 tensor with K <= "
                                     f"{_lib.OCCLUSION_MAX_OUTPUTS} for one patient, got {tuple(outputs.shape)} {outputs.dtype}")
                base = outputs.contiguous()
                k = int(base.shape[1])
                if self.fill == "mean":
                    fill = torch.empty(c, device=dev, dtype=torch.float32)
                    ws = torch.empty(c * _lib.CHANNEL_MEANS_PARTS, device=dev, dtype=torch.float64)
                    _lib.enqueue("mmnn_channel_means", image.data_ptr(), c, d * h * w, fill.data_ptr(), ws.data_ptr())
                else:
                    fill = torch.full((c,), self.fill, device=dev, dtype=torch.float32)
                scores = torch.empty((wn, k), device=dev, dtype=torch.float32)
                occluded = torch.empty((self.batch, c, d, h, w), device=dev, dtype=torch.float32)
                clinical = x["clinical"].expand(self.batch, -1).contiguous() if self.multimodal else None
                for first in range(0, wn, self.batch):
                    _lib.enqueue("mmnn_occlude_windows", ctypes.byref(desc), image.data_ptr(), fill.data_ptr(), first, self.batch, occluded.data_ptr())
                    out = m({"image": occluded, "clinical": clinical} if self.multimodal else occluded)
                    rows = min(self.batch, wn - first)                  # the padded tail of the last batch repeats the last window
                    scores[first:first + rows].copy_(out[:rows])
                maps = torch.empty((k, d, h, w), device=dev, dtype=torch.float32)
                _lib.enqueue("mmnn_occlusion_map", ctypes.byref(desc), k, base.data_ptr(), scores.data_ptr(), maps.data_ptr())
                self.scores = scores
        finally:
            for mod, mode in modes:
                mod.training = mode
        return outputs, maps


def add_occlusion(model, multimodal=False, **kw):
    """The twin of `add_gradcam`: an `OcclusionSensitivity` over the fusion model (multimodal) or an image-only one; `kw` are its
    window / stride / batch / fill."""
    return OcclusionSensitivity(model, multimodal=multimodal, **kw)


class Normalize:
    """utils/utils.py:348-355: (x - mean * max(x)) / (std * max(x)), max over the whole sample (all channels); the sign of max(x) is
    kept.  A stage of mmnn_sts_amd.transforms.Compose; called on its own it runs as a one-stage pipeline on the device."""
    bit = 1          # transforms.NORMALIZE
    prob = None

    def __init__(self, mean, std):
        if float(std) == 0.0:
            raise ValueError("Normalize: std must be non-zero")
        self.mean = float(mean)
        self.stddev = float(std)

    def __call__(self, image):
        from ..transforms import Compose
        return Compose([self])(image)


def remap_bhb_keys(entries):
    """Key translation of the BHB-10K pretrained DenseNet121 checkpoint (utils/utils.py:368-384): drop the DataParallel prefix and
    address a dense layer's leaves through its `layers` Sequential.  (The result still says `features.*` where this DenseNet says
    `backbone.*` -- SURVEY Appendix A Q13 -- so with strict=False the convolutional weights match nothing, exactly as upstream.)"""
    out = {}
    for key, value in entries.items():
        parts = key.replace('module.', '').split('.')
        if parts[0] == 'features' and len(parts) > 1 and parts[1].startswith('dense'):
            parts.insert(3, 'layers')
        out['.'.join(parts)] = value
    return out


def loadWeights(model, path, device):
    """utils/utils.py:357-390 for local files: plain state_dict, or the BHB-10K pretrained DenseNet121 key remap."""
    checkpoint = torch.load(path, map_location=device)
    if isinstance(checkpoint, dict) and 'model' in checkpoint and path.endswith('DenseNet121_BHB-10K_yAwareContrastive.pth'):
        model.load_state_dict(remap_bhb_keys(checkpoint['model']), strict=False)
        logger.info('Loaded pretrained backbone')
    else:
        model.load_state_dict(checkpoint)
        logger.info('Loaded provided weights from disk')
    return model
