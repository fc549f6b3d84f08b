#!/usr/bin/env python
"""Time of the image-only Grad-CAM (utils.GradCAM) against the eval forward alone, with HIP events after warm-up.

    python tools/gradcam_unimodal_time.py [--steps 20] [--warmup 3] [--case I] [--json out.json]

Per case: `forward_ms` = the model's eval forward under no_grad, `cam_ms` = cam(x) (forward + Grad-CAM), and `after_forward_us` = the
Grad-CAM part alone (`GradCAM._attention`: the one C-ABI call -- head, count, heat, normalise kernels and the up-sampling -- on the
captured tensors of the last forward), each call queued back to back behind a spin kernel so that the device time is measured rather
than the host's launch pace.  `maps_write_tbs` prices the attention maps' bytes (written once) over that whole Grad-CAM time: a
lower bound of the up-sampler's own rate, which a `rocprofv3 --kernel-trace --stats` run of this tool gives per kernel.
Cases: DenseNet121 (one channel) at 1x1x256^3 and 4x1x128^3, r3d_18 at 4x1x128^3."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd.models.densenet import DenseNet121  # noqa: E402
from mmnn_sts_amd.models.resnet import r3d_18  # noqa: E402
from mmnn_sts_amd.utils.utils import GradCAM  # noqa: E402

CASES = (("densenet121", (1, 1, 256, 256, 256)), ("densenet121", (4, 1, 128, 128, 128)), ("r3d_18", (4, 1, 128, 128, 128)))


def build(name):
    torch.manual_seed(0)
    if name == "densenet121":
        return DenseNet121(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, dropout_prob=0.2).cuda().eval()
    return r3d_18(2).cuda().eval()


def events_ms(fn, steps):
    """Median of per-call times between events, every call queued behind a spin so that the device never waits for the host."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda._sleep(50_000_000)
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def time_case(name, shape, steps, warmup):
    model = build(name)
    x = torch.randn(shape, device="cuda")
    cam = GradCAM(model)
    with torch.no_grad():
        for _ in range(warmup):
            model(x)
            cam(x)
        torch.cuda.synchronize()
        fwd = events_ms(lambda: model(x), steps)
        full = events_ms(lambda: cam(x), steps)
        captured = cam._densenet(x) if cam.kind == "densenet" else cam._r3d(x)
        for _ in range(warmup):
            cam._attention(captured, shape[2:])
        after = events_ms(lambda: cam._attention(captured, shape[2:]), steps)
    maps_bytes = 4 * shape[0] * shape[2] * shape[3] * shape[4]
    return {"model": name, "shape": list(shape), "captured": list(cam.features.shape), "forward_ms": round(fwd, 4),
            "cam_ms": round(full, 4), "after_forward_us": round(after * 1e3, 2),
            "after_forward_share_of_forward": round(after / fwd, 5), "maps_write_tbs": round(maps_bytes / (after * 1e-3) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", type=int, default=None, help="index into CASES: one case only (a kernel-statistics run per case)")
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gradcam_unimodal_time.py measures on the MI355X; no GPU found")
    cases = CASES if a.case is None else CASES[a.case:a.case + 1]
    rows = [time_case(n, s, a.steps, a.warmup) for n, s in cases]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
