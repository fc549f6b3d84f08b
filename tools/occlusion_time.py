#!/usr/bin/env python
"""Time of occlusion sensitivity for one patient at the defaults (csrc/occlusion.hip, utils.OcclusionSensitivity): a 2 x 64^3 input,
window 16, stride 8 -> 343 windows, 43 batches of 8 through the default fusion model (DenseNet121 + clinical MLP).

    python tools/occlusion_time.py [--steps 50] [--warmup 10] [--repeats 3] [--json profiles/occlusion_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone), as in
tools/seg_time.py; every figure is the median of `repeats` windows of `steps` calls:
    occlude_us                   `mmnn_occlude_windows` for one batch of 8 (16.8 MB written, the 2.1 MB input read once from HBM at most),
                                 the same output buffer every call (it stays in the 256 MB last-level cache: the warm figure)
    occlude_rotating_us          ... with 24 output buffers in turn (403 MB: every call writes lines the cache no longer holds)
    channel_means_us             `mmnn_channel_means` of the input (both launches)
    occlusion_map_us             `mmnn_occlusion_map`: 343 x 2 scores -> 2 x 64^3
    forward_batch_us             the model's eval forward of one occluded batch of 8
    forward_single_us            ... of the unoccluded patient (batch 1)
    patient_ms                   `OcclusionSensitivity(model)(x)` end to end, wall clock around a synchronised call
The bytes `mmnn_occlude_windows` moves (the batch written once, the input and the fill read once) are priced against the 6.29 TB/s
measured HBM ceiling; the share of the patient's time spent inside the model's forwards is (43 forward_batch + forward_single) /
patient."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import _lib  # noqa: E402
from mmnn_sts_amd.models.densenet import DenseNet121  # noqa: E402
from mmnn_sts_amd.models.multimodal import MultiModalModel  # noqa: E402
from mmnn_sts_amd.utils.utils import OcclusionSensitivity  # noqa: E402

HBM_TBS = 6.29
C, S, WINDOW, STRIDE, BATCH = 2, 64, 16, 8, 8
ROTATING = 24


def queued_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="every figure is the median of this many windows of --steps calls")
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "occlusion_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    x = torch.randn((1, C, S, S, S), device="cuda")
    clinical = torch.randn((1, 32), device="cuda")
    model = MultiModalModel(DenseNet121(spatial_dims=3, in_channels=C, out_channels=2, feature_channels=12, dropout_prob=0.2),
                            [f"predictor{i}" for i in range(32)], 2, 12, blend=False).to("cuda").eval()
    desc = _lib.OcclusionDesc(C, S, S, S, (ctypes.c_int32 * 3)(WINDOW, WINDOW, WINDOW), (ctypes.c_int32 * 3)(STRIDE, STRIDE, STRIDE))
    wn = L.mmnn_occlusion_window_count(ctypes.byref(desc), None)
    assert wn == 343, wn
    batches = -(-wn // BATCH)
    fill = torch.empty(C, device="cuda")
    ws = torch.empty(C * _lib.CHANNEL_MEANS_PARTS, dtype=torch.float64, device="cuda")
    outs = [torch.empty((BATCH, C, S, S, S), device="cuda") for _ in range(ROTATING)]
    base = torch.randn(2, device="cuda")
    scores = torch.randn((wn, 2), device="cuda")
    maps = torch.empty((2, S, S, S), device="cuda")
    turn = [0]

    def means():
        _lib.check(L.mmnn_channel_means(x.data_ptr(), C, S * S * S, fill.data_ptr(), ws.data_ptr(), stream), "mmnn_channel_means")

    def occlude():
        _lib.check(L.mmnn_occlude_windows(ctypes.byref(desc), x.data_ptr(), fill.data_ptr(), 171, BATCH, outs[0].data_ptr(), stream),
                   "mmnn_occlude_windows")

    def occlude_rotating():
        turn[0] = (turn[0] + 1) % ROTATING
        _lib.check(L.mmnn_occlude_windows(ctypes.byref(desc), x.data_ptr(), fill.data_ptr(), 171, BATCH, outs[turn[0]].data_ptr(), stream),
                   "mmnn_occlude_windows")

    def assemble():
        _lib.check(L.mmnn_occlusion_map(ctypes.byref(desc), 2, base.data_ptr(), scores.data_ptr(), maps.data_ptr(), stream), "mmnn_occlusion_map")

    clinical8 = clinical.expand(BATCH, -1).contiguous()

    def forward_batch():
        with torch.no_grad():
            return model({"image": outs[0], "clinical": clinical8})

    def forward_single():
        with torch.no_grad():
            return model({"image": x, "clinical": clinical})

    means()
    occlude()
    occ = OcclusionSensitivity(model, window=WINDOW, stride=STRIDE, batch=BATCH, multimodal=True)
    arg = {"image": x, "clinical": clinical}

    def patient():
        torch.cuda.synchronize()
        t = time.perf_counter()
        occ(arg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(2):
        patient()
    patient_ms = [patient() for _ in range(max(3, a.repeats))]
    named = (("occlude_us", occlude), ("occlude_rotating_us", occlude_rotating), ("channel_means_us", means), ("occlusion_map_us", assemble),
             ("forward_batch_us", forward_batch), ("forward_single_us", forward_single))
    for _, fn in named:
        for _ in range(a.warmup):
            fn()
    runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]
    times = {name: round(float(np.median([r[name] for r in runs])), 1) for name, _ in named}
    spread = {name: [round(min(r[name] for r in runs), 1), round(max(r[name] for r in runs), 1)] for name, _ in named}
    written = 4 * BATCH * C * S ** 3
    read = 4 * C * S ** 3 + 4 * C
    moved = written + read
    p_ms = float(np.median(patient_ms))
    forwards_ms = (batches * times["forward_batch_us"] + times["forward_single_us"]) / 1e3
    res = {"input": [C, S, S, S], "window": WINDOW, "stride": STRIDE, "batch": BATCH, "windows": int(wn), "batches": batches,
           "model": "MultiModalModel(DenseNet121, 32 clinical predictors), eval", "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           **times, "min_max_over_repeats": spread, "occlude_write_MB": round(written / 1e6, 2), "occlude_read_MB": round(read / 1e6, 2),
           "occlude_hbm_floor_us": round(moved / (HBM_TBS * 1e12) * 1e6, 2),
           "occlude_share_of_hbm_ceiling": round(moved / (times["occlude_us"] * 1e-6) / 1e12 / HBM_TBS, 3),
           "occlude_rotating_share_of_hbm_ceiling": round(moved / (times["occlude_rotating_us"] * 1e-6) / 1e12 / HBM_TBS, 3),
           "patient_ms": round(p_ms, 1), "patient_ms_min_max": [round(min(patient_ms), 1), round(max(patient_ms), 1)],
           "forwards_ms": round(forwards_ms, 1), "forwards_share_of_patient": round(forwards_ms / p_ms, 3),
           "occlude_all_batches_ms": round(batches * times["occlude_us"] / 1e3, 2)}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
