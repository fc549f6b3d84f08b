"""Time per iteration of the learning-rate range test.

    python tools/time_lr_finder.py --leg new        # LRFinder.range_test: the sweep enqueued without host waits
    python tools/time_lr_finder.py --leg baseline   # torch-lr-finder's loop: torch CrossEntropyLoss, FusedSGD.step() with a
                                                    # host lr, loss.item() every iteration (runs unchanged on older trees)

Both legs: DenseNet121 (3 classes) on batches of 2 x 1 x 64^3 after the device train transforms, end_lr 1e-3 (nothing stops
early), `--iters` iterations, `--reps` timed repetitions after one warm-up sweep, each from the same initial state.  Prints one
JSON line: per-repetition ms per iteration, their median and max - min spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmnn_sts_amd.models.densenet import DenseNet121  # noqa: E402
from mmnn_sts_amd.optim import FusedSGD  # noqa: E402
from mmnn_sts_amd.transforms import train_transforms  # noqa: E402


def make_batches(dev_seed=5):
    g = torch.Generator().manual_seed(dev_seed)
    x = torch.randn((6, 1, 64, 64, 64), generator=g)
    y = (torch.rand((6, 3), generator=g) < 0.6).float()
    return [(x[i:i + 2].clone().pin_memory(), y[i:i + 2].clone().pin_memory()) for i in range(0, 6, 2)]


def baseline_sweep(model, opt, batches, num_iter, end_lr, dev, smooth_f=0.05, diverge_th=5):
    crit = torch.nn.CrossEntropyLoss()
    base = float(opt.param_groups[0]["lr"])
    model.train()
    hist, best = [], None
    it = iter(batches)
    for i in range(num_iter):
        lr = base * (end_lr / base) ** (i / (num_iter - 1))
        opt.zero_grad()
        try:
            x, y = next(it)
        except StopIteration:
            it = iter(batches)
            x, y = next(it)
        x = train_transforms(x.to(dev, non_blocking=True))
        loss = crit(model(x), y.to(dev, non_blocking=True))
        loss.backward()
        opt.param_groups[0]["lr"] = lr
        opt.step()
        raw = loss.item()
        s = raw if i == 0 else smooth_f * raw + (1 - smooth_f) * hist[-1]
        best = s if best is None or s < best else best
        hist.append(s)
        if s > diverge_th * best:
            break
    return len(hist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("new", "baseline"), required=True)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--end_lr", type=float, default=1e-3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = DenseNet121(spatial_dims=3, in_channels=1, out_channels=3, feature_channels=64, dropout_prob=0.0).to(dev)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    batches = make_batches()
    train_transforms.set_random_state(0)

    def fresh_opt():
        model.load_state_dict(sd0)
        return FusedSGD(model, 1e-7, momentum=0.9, nesterov=True, weight_decay=1e-4)

    if a.leg == "new":
        from mmnn_sts_amd.losses.losses import CrossEntropyLoss
        from mmnn_sts_amd.utils.find_lr import LRFinder

        def sweep(n):
            f = LRFinder(model, fresh_opt(), CrossEntropyLoss(), device=dev)
            f.range_test(batches, end_lr=a.end_lr, num_iter=n, transform=train_transforms)
            return f.iters_done
    else:
        def sweep(n):
            return baseline_sweep(model, fresh_opt(), batches, n, a.end_lr, dev)

    sweep(max(2, a.iters // 5))                   # warm-up: plans, workspaces, kernel attributes
    times, done = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done.append(sweep(a.iters))
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / a.iters)
    print(json.dumps({"leg": a.leg, "iters": a.iters, "iters_done": done, "ms_per_iter": [round(t, 4) for t in times],
                      "median_ms_per_iter": round(statistics.median(times), 4), "spread_ms": round(max(times) - min(times), 4),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
