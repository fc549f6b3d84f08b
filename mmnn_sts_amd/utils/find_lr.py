"""Learning-rate range test of upstream's `utils/find_lr.py` (torch-lr-finder's `LRFinder.range_test` + `plot` + `reset`), with the
sweep resident on the device.

Every iteration of the sweep is enqueued without waiting on the GPU: the loss, its smoothing, the best loss and the divergence stop
are kept in a small device struct (`mmnn_lr_range_*`), the learning rate of iteration i is read by the SGD kernels from a device
table (`FusedSGD.step_device_lr`), and a stop switches the update off on the device (`live`).  The host only polls `live` through a
pinned word every `poll_every` iterations to stop enqueueing, and reads the history once at the end.  The arithmetic restates
torch-lr-finder 0.2.x: fp32 loss sum, fp64 exponential smoothing, `s > diverge_th * best` stops.
"""
import collections
import logging
import os
import random

import numpy as np
import torch

from .. import _lib
from ..losses.losses import CrossEntropyLoss
from ..optim import FusedSGD

logger = logging.getLogger(__name__)


def lr_schedule(base_lr: float, end_lr: float, num_iter: int, step_mode: str = "exp"):
    """torch-lr-finder's ExponentialLR / LinearLR value at every iteration i (r = i / (num_iter - 1), Python doubles)."""
    out = []
    for i in range(num_iter):
        out.append(_schedule_value(base_lr, end_lr, num_iter, step_mode, i))
    return out


def _schedule_value(base_lr, end_lr, num_iter, step_mode, i):
    r = i / (num_iter - 1)
    if step_mode == "exp":
        return base_lr * (end_lr / base_lr) ** r
    return base_lr + r * (end_lr - base_lr)


def suggest_lr(history, skip_start: int = 10, skip_end: int = 5):
    """`plot(suggest_lr=True)`: the lr at the steepest descent of the recorded loss (np.gradient argmin) after trimming; None when
    fewer than 2 points remain."""
    lrs, losses = history["lr"], history["loss"]
    if skip_end == 0:
        lrs, losses = lrs[skip_start:], losses[skip_start:]
    else:
        lrs, losses = lrs[skip_start:-skip_end], losses[skip_start:-skip_end]
    if len(losses) < 2:
        logger.info("Failed to compute the gradients, there might not be enough points.")
        return None
    idx = int(np.gradient(np.array(losses)).argmin())
    return lrs[idx]


_suggest_lr = suggest_lr      # LRFinder.plot's `suggest_lr` flag shadows the name


def split_uids(uids, seed):
    """Upstream's split: random.seed(seed); random.shuffle(uids); the first round(0.8 n) train, the rest validate."""
    uids = list(uids)
    random.seed(seed)
    random.shuffle(uids)
    k = round(len(uids) * 0.8)
    return uids[:k], uids[k:]


class LRFinder:
    """torch-lr-finder's LRFinder for this package's `FusedSGD` and `CrossEntropyLoss` (the pair upstream's find_lr builds)."""

    def __init__(self, model, optimizer, criterion, device=None):
        if not isinstance(optimizer, FusedSGD):
            raise TypeError("LRFinder needs an mmnn_sts_amd.optim.FusedSGD optimizer (its learning rate is read from device memory)")
        if not isinstance(criterion, CrossEntropyLoss):
            raise TypeError("LRFinder needs an mmnn_sts_amd.losses.losses.CrossEntropyLoss criterion")
        self.model, self.optimizer, self.criterion = model, optimizer, criterion
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.history = {"lr": [], "loss": []}
        self.best_loss = None
        self.stop_iter = None
        self.iters_done = 0
        self.iters_enqueued = 0
        # state to restore on reset(): parameters, buffers (running statistics, num_batches_tracked), optimizer state
        self._model_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        self._opt_state = optimizer.snapshot_state()

    def reset(self):
        self.model.load_state_dict(self._model_state)
        for m in self.model.modules():
            if hasattr(m, "mark_params_changed"):
                m.mark_params_changed()
        self.optimizer.restore_state(self._opt_state)

    def range_test(self, train_loader, val_loader=None, start_lr=None, end_lr=10, num_iter=100, step_mode="exp", smooth_f=0.05,
                   diverge_th=5, accumulation_steps=1, transform=None, poll_every=10, max_ahead="default"):
        """Enqueue up to `num_iter` iterations of forward, loss, backward and SGD step at the scheduled learning rates.  `transform`
        (optional) is applied to every input batch on the device.  `poll_every`: iterations between non-blocking polls of the stop
        flag; `max_ahead` (default 2 * poll_every, None: unbounded): at most this many iterations are enqueued beyond the newest
        completed poll, so at most this many iterations are wasted after a stop."""
        if val_loader is not None:
            raise NotImplementedError("LRFinder.range_test: val_loader mode is not provided")
        if step_mode.lower() not in ("exp", "linear"):
            raise ValueError(f"expected one of (exp, linear), got {step_mode}")
        step_mode = step_mode.lower()
        if num_iter <= 1:
            raise ValueError("`num_iter` must be larger than 1")
        if smooth_f < 0 or smooth_f >= 1:
            raise ValueError("smooth_f is outside the range [0, 1[")
        if poll_every < 1:
            raise ValueError("poll_every must be at least 1")
        if max_ahead == "default":
            max_ahead = 2 * poll_every
        if max_ahead is not None and max_ahead < poll_every:
            raise ValueError(f"max_ahead ({max_ahead}) must be None or at least poll_every ({poll_every})")
        if start_lr is not None:
            for g in self.optimizer.param_groups:
                g["lr"] = start_lr
        base_lr = float(self.optimizer.param_groups[0]["lr"])
        lrs = lr_schedule(base_lr, end_lr, num_iter, step_mode)
        self.history = {"lr": [], "loss": []}
        dev = self.device
        table = torch.tensor(lrs, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)   # rounded to fp32 once, as ctypes does
        state = torch.empty((_lib.lib().mmnn_lr_range_state_bytes(num_iter),), dtype=torch.uint8, device=dev)
        _lib.enqueue("mmnn_lr_range_init", state.data_ptr(), num_iter, device=dev)
        live = state[_lib.LRS_LIVE:_lib.LRS_LIVE + 4].view(torch.int32)
        n_polls = num_iter // poll_every + 1
        words = torch.ones((n_polls,), dtype=torch.int32).pin_memory()
        words_np = words.numpy()
        pending = collections.deque()             # (iteration, poll slot, event), oldest first
        newest_seen = 0                            # iterations known to have completed (from the newest finished poll)
        stopped = False
        data = iter(train_loader)
        one_minus = 1 - smooth_f
        self.model.train()
        i = 0

        def settle(entry):
            nonlocal newest_seen, stopped
            it, slot, _ = entry
            newest_seen = it + 1
            if words_np[slot] == 0:
                stopped = True

        while i < num_iter:
            while pending and pending[0][2].query():
                settle(pending.popleft())
            if stopped:
                break
            # host too far ahead of the GPU: block on the oldest poll (the only waits of the sweep, at most one per poll).  A stop at
            # iteration s is seen by the first poll after it, so at most `max_ahead` iterations are enqueued past s + 1.
            while max_ahead is not None and i - newest_seen > max_ahead and pending and not stopped:
                entry = pending.popleft()
                entry[2].synchronize()
                settle(entry)
            if stopped:
                break
            self.optimizer.zero_grad()
            for a in range(accumulation_steps):
                try:
                    x, y = next(data)
                except StopIteration:
                    data = iter(train_loader)
                    x, y = next(data)
                x, y = _to_device(x, dev), _to_device(y, dev)
                if transform is not None:
                    x = transform(x)
                loss = self.criterion(self.model(x), y)
                if accumulation_steps > 1:
                    loss = loss / accumulation_steps
                loss.backward()
                _lib.enqueue("mmnn_lr_range_accumulate", state.data_ptr(), loss.detach().data_ptr(), 1.0, int(a == 0), device=dev)
            self.optimizer.step_device_lr(table[i:i + 1], live)
            _lib.enqueue("mmnn_lr_range_update", state.data_ptr(), i, float(smooth_f), float(one_minus), float(diverge_th), device=dev)
            i += 1
            if i % poll_every == 0:
                slot = i // poll_every
                words[slot:slot + 1].copy_(live, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending.append((i - 1, slot, ev))
        self.iters_enqueued = i
        host = state.cpu()                          # the one blocking readback
        ints = host[:_lib.LRS_BEST].view(torch.int32)
        stop_iter = int(ints[_lib.LRS_STOP_ITER // 4])
        self.iters_done = int(ints[_lib.LRS_ITERS_DONE // 4])
        self.stop_iter = stop_iter if stop_iter >= 0 else None
        hist = host[_lib.LRS_HIST:].view(torch.float64).numpy()
        self.best_loss = float(host[_lib.LRS_BEST:_lib.LRS_HIST].view(torch.float64)[0])
        k = self.iters_done
        self.history = {"lr": lrs[:k], "loss": [float(v) for v in hist[:k]]}
        # the group lr upstream's scheduler leaves: the schedule value at the index after the last iteration
        for g in self.optimizer.param_groups:
            g["lr"] = _schedule_value(base_lr, end_lr, num_iter, step_mode, k)
        if self.stop_iter is not None:
            print("Stopping early, the loss has diverged")
        print("Learning rate search finished. See the graph with {finder_name}.plot()")

    def plot(self, skip_start=10, skip_end=5, log_lr=True, show_lr=None, ax=None, suggest_lr=True, path="lr_finder.png"):
        """The suggestion (steepest descent of the smoothed loss) and, when matplotlib imports, the loss-vs-lr graph in `path`."""
        if skip_start < 0 or skip_end < 0:
            raise ValueError("skip_start and skip_end cannot be negative")
        suggestion = _suggest_lr(self.history, skip_start, skip_end) if suggest_lr else None
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            return suggestion
        lrs, losses = self.history["lr"], self.history["loss"]
        lrs, losses = (lrs[skip_start:], losses[skip_start:]) if skip_end == 0 else (lrs[skip_start:-skip_end], losses[skip_start:-skip_end])
        fig, axis = plt.subplots()
        axis.plot(lrs, losses)
        if log_lr:
            axis.set_xscale("log")
        axis.set_xlabel("Learning rate")
        axis.set_ylabel("Loss")
        if suggestion is not None:
            axis.scatter([suggestion], [losses[lrs.index(suggestion)]], s=75, marker="o", color="red", zorder=3, label="steepest gradient")
            axis.legend()
        if show_lr is not None:
            axis.axvline(x=show_lr, color="red")
        if path:
            fig.savefig(path)
        plt.close(fig)
        return suggestion


def _to_device(t, dev):
    if not t.is_pinned():
        t = t.pin_memory()
    return t.to(dev, non_blocking=True)


class _ImageLabels(torch.utils.data.Dataset):
    """(image, event flags as float probability targets) of the given uids of a dataset with `images` / `events`."""

    def __init__(self, dataset, uids):
        self.dataset, self.uids = dataset, list(uids)

    def __len__(self):
        return len(self.uids)

    def __getitem__(self, i):
        x, ev = self.dataset[self.uids[i]][:2]
        return x.float(), ev.float()


def find_lr(args, dataset):
    """Upstream utils/find_lr.py:27-112 on an image classification dataset (`dataset.uids`, `dataset[uid] -> (image, events, ...)`).
    Returns (finder, suggested lr).  `args`: seed, batch_size, output_path, optional in_channels, num_iter, end_lr."""
    from ..models.densenet import densenet121
    from ..transforms import train_transforms
    device = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    train_uids, val_uids = split_uids(dataset.uids, args.seed)
    out = getattr(args, "output_path", ".")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "train_uids.txt"), "w") as f:
        f.write("\n".join(str(x) for x in train_uids))
    with open(os.path.join(out, "val_uids.txt"), "w") as f:
        f.write("\n".join(str(x) for x in val_uids))
    train_dataset = _ImageLabels(dataset, train_uids)
    print("Training count =", len(train_dataset), "Validation count =", len(val_uids))
    train_loader = torch.utils.data.DataLoader(train_dataset, batch_size=args.batch_size, shuffle=True, pin_memory=True)
    in_channels = getattr(args, "in_channels", None) or train_dataset[0][0].shape[0]
    model = densenet121(spatial_dims=3, in_channels=in_channels, out_channels=3).to(device)
    loss_function = CrossEntropyLoss()
    optimizer = FusedSGD(model, 1e-7, momentum=0.9, nesterov=True, weight_decay=1e-4)
    finder = LRFinder(model, optimizer, loss_function, device=device)
    finder.range_test(train_loader, end_lr=getattr(args, "end_lr", 100), num_iter=getattr(args, "num_iter", 100), transform=train_transforms)
    suggestion = finder.plot(path=os.path.join(out, "lr_finder.png"))
    finder.reset()
    return finder, suggestion
