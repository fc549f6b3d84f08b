#!/usr/bin/env python
"""Time of the input transforms (mmnn_sts_amd/transforms.py) per batch, with HIP events after warm-up: `device_us_per_batch` with
the batches queued back to back behind a spin kernel (device time alone), `call_us_per_batch` between events around each call
(includes the host's packing and launch pace when the device outruns it).

    python tools/transforms_time.py [--steps 50] [--warmup 10] [--json out.json]

Cases: train_transforms on (2,2,64^3) -- upstream's real input, its dataset already resizes to 64^3 -- and on (2,2,128^3) -> 64^3,
each with upstream's probabilities (fresh draws every batch, mean over the batches) and with every stage forced on; val_transforms
on both inputs.  Bytes are the algorithmic HBM traffic of the passes that ran (each pass reads its input once and writes its output
once; the sharpen's last pass also reads the blurred volume), priced against the 6.29 TB/s measured HBM ceiling of the MI355X."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import transforms as T  # noqa: E402

HBM_TBS = 6.29


def pass_bytes(stages, fire_any, shape, out_ext):
    """HBM bytes of the passes mmnn_transform_volumes launches for one group (csrc/transforms.hip, host orchestration)."""
    n, c, d, h, w = shape
    I = 4 * n * c * d * h * w
    O = 4 * n * c * out_ext[0] * out_ext[1] * out_ext[2]
    b = 0
    pend = bool(stages & (T.NORMALIZE | T.SCALE))
    if pend:
        b += I                                   # min / max of the raw input
    resize = (stages & T.RESIZE) and (d, h, w) != tuple(out_ext)
    wrote_out = False                            # whether a pass has written `out` yet
    if fire_any & (T.ROTATE | T.FLIP):
        b += 2 * I; pend = False; wrote_out = not (fire_any & T.ZOOM) and not resize
    if fire_any & T.ZOOM:
        b += 2 * I; pend = False; wrote_out = not resize
    if resize:
        b += I + O; pend = False; wrote_out = True
    if fire_any & (T.SMOOTH | T.SHARPEN):
        if fire_any & (T.SHIFT | T.CONTRAST) or pend:
            b += 2 * O; pend = False
        if fire_any & T.SMOOTH:
            b += 6 * O
        if fire_any & T.SHARPEN:
            b += 13 * O
        wrote_out = True
        if fire_any & (T.HIST | T.NOISE):
            b += 2 * O
    elif fire_any & (T.SHIFT | T.CONTRAST | T.HIST | T.NOISE):
        b += 2 * O; pend = False; wrote_out = True
    if pend or not wrote_out:
        b += 2 * O                               # the folded affine / copy into `out`
    return b


def time_case(tf, shape, steps, warmup, force_all):
    x = (300.0 + 200.0 * torch.randn(shape, device="cuda")).abs()
    tf.set_random_state(1234)
    n = shape[0]
    plans = []
    for _ in range(warmup + steps):
        ps = tf.randomize(n)
        if force_all:
            for p in ps:
                p.fire = tf.stages
        plans.append(ps)
    for ps in plans[:warmup]:
        tf.apply(x, ps)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for (a, b), ps in zip(ev, plans[warmup:]):
        a.record()
        tf.apply(x, ps)
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    # device time alone: the same batches queued behind a ~20 ms spin, so that they run back to back whatever the host's pace
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    a.record()
    for ps in plans[warmup:]:
        tf.apply(x, ps)
    b.record()
    torch.cuda.synchronize()
    dev_ms = a.elapsed_time(b) / steps
    nbytes = []
    for ps in plans[warmup:]:
        fire_any = 0
        for p in ps:
            fire_any |= p.fire & tf.stages
        nbytes.append(pass_bytes(tf.stages, fire_any, shape, tf.spatial_size or shape[2:]))
    mean_b = sum(nbytes) / len(nbytes)
    floor_s = mean_b / (HBM_TBS * 1e12)
    return {"device_us_per_batch": round(dev_ms * 1e3, 1), "call_us_per_batch": round(sum(ms) / len(ms) * 1e3, 1), "MB": round(mean_b / 1e6, 2),
            "GBps": round(mean_b / (dev_ms * 1e-3) / 1e9, 1), "hbm_floor_us": round(floor_s * 1e6, 1), "x_floor": round(dev_ms * 1e-3 / floor_s, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {}
    for name, tf, shape, force in (("train_64_upstream_probs", T.train_transforms, (2, 2, 64, 64, 64), False),
                                   ("train_64_all_on", T.train_transforms, (2, 2, 64, 64, 64), True),
                                   ("train_128_to_64_upstream_probs", T.train_transforms, (2, 2, 128, 128, 128), False),
                                   ("train_128_to_64_all_on", T.train_transforms, (2, 2, 128, 128, 128), True),
                                   ("val_64", T.val_transforms, (2, 2, 64, 64, 64), False),
                                   ("val_128_to_64", T.val_transforms, (2, 2, 128, 128, 128), False)):
        res[name] = time_case(tf, shape, a.steps, a.warmup, force)
        print(json.dumps({"case": name, **res[name]}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
