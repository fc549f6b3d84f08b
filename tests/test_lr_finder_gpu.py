"""The learning-rate range test on the MI355X (upstream utils/find_lr.py -> torch-lr-finder's LRFinder):
the native cross entropy against torch in fp64, the device-resident sweep bookkeeping against a Python restatement (bit for bit),
the device-lr SGD against the host-lr kernels (bit for bit), LRFinder.range_test against a host-driven loop (bit for bit), the
absence of host waits inside the sweep, and `main.py --lr_finder` end to end."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._cli import run_main

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. cross entropy against torch (fp64 oracle on CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def _logits(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((n, c), generator=g) * 3
    for r in range(n):
        if r % 3 == 1:                                  # wide spread: +-80
            z[r] = (torch.rand((c,), generator=g) * 2 - 1) * 80
            z[r, r % c] = 80.0
            z[r, (r + 1) % c] = -80.0
        elif r % 3 == 2:                                # ties
            z[r] = torch.round(z[r])
            z[r, 0] = z[r, c - 1]
    return z.float()


def _targets(n, c, kind, seed):
    g = torch.Generator().manual_seed(seed + 1)
    if kind == "index":
        y = torch.randint(0, c, (n,), generator=g)
        if n > 1:
            y[1::3] = -100                              # ignored rows
        return y
    y = (torch.rand((n, c), generator=g) < 0.5).float()     # multi-hot event flags
    if n > 1:
        y[1] = 0.0                                      # all-zero row
    if n > 2:
        p = torch.rand((c,), generator=g)
        y[2] = p / p.sum()                              # a soft probability row
    return y


def _err(a, ref):
    return float((a.double() - ref).abs().max())


CE_CASES = [(n, c, kind, red) for n in (1, 2, 7, 300) for c in (2, 3, 17) for kind in ("index", "prob") for red in ("none", "sum", "mean")]


@pytest.mark.parametrize("n,c,kind,red", CE_CASES)
def test_cross_entropy_against_torch(n, c, kind, red):
    """Loss and gradient (through autograd, non-unit upstream gradient) against F.cross_entropy in fp64 on the same fp32 logits.
    Bound per case: 4x the error of torch's own CPU fp32 result against the same fp64 oracle, floor 2^-22 * max|value|."""
    from mmnn_sts_amd.losses.losses import CrossEntropyLoss
    seed = n * 1000 + c * 10 + (kind == "prob")
    z = _logits(n, c, seed)
    y = _targets(n, c, kind, seed)
    up = (torch.rand((n,), generator=torch.Generator().manual_seed(seed + 2)) * 2 - 0.5) if red == "none" else torch.tensor(0.7)

    def run(zz, yy, uu, fn):
        zz = zz.clone().requires_grad_(True)
        loss = fn(zz, yy)
        loss.backward(uu)
        return loss.detach(), zz.grad

    ref_l, ref_g = run(z.double(), y.double() if kind == "prob" else y, up.double(), lambda a, b: F.cross_entropy(a, b, reduction=red))
    t32_l, t32_g = run(z, y, up, lambda a, b: F.cross_entropy(a, b, reduction=red))
    crit = CrossEntropyLoss(reduction=red)
    our_l, our_g = run(z.to(DEV), y.to(DEV), up.to(DEV), crit)
    our_l, our_g = our_l.cpu(), our_g.cpu()
    assert our_l.shape == ref_l.shape and our_g.shape == ref_g.shape
    for what, ours, t32, ref in (("loss", our_l, t32_l, ref_l), ("grad", our_g, t32_g, ref_g)):
        e_ours, e_t32 = _err(ours, ref), _err(t32, ref)
        tol = max(4 * e_t32, 2.0 ** -22 * float(ref.abs().max()))
        print(f"CE n={n} c={c} {kind} {red} {what}: ours {e_ours:.3e} torch-fp32 {e_t32:.3e} bound {tol:.3e}")
        assert e_ours <= tol, (what, e_ours, e_t32, tol)


def test_cross_entropy_edge_cases():
    """All rows ignored -> NaN mean; an out-of-range index -> a NaN row (loss and gradient), no fault; two calls are bit-identical."""
    from mmnn_sts_amd.losses.losses import CrossEntropyLoss
    z = _logits(5, 3, 7).to(DEV)
    ign = torch.full((5,), -100, dtype=torch.int64, device=DEV)
    assert torch.isnan(CrossEntropyLoss()(z, ign)).item()
    bad = torch.tensor([0, 3, 2, -7, 1], device=DEV)
    zz = z.clone().requires_grad_(True)
    loss = CrossEntropyLoss(reduction="none")(zz, bad)
    loss.sum().backward()
    torch.cuda.synchronize()
    l, g = loss.detach().cpu(), zz.grad.cpu()
    ok = torch.tensor([True, False, True, False, True])
    assert torch.isnan(l[~ok]).all() and torch.isfinite(l[ok]).all()
    assert torch.isnan(g[~ok]).all() and torch.isfinite(g[ok]).all()
    ref = F.cross_entropy(z.cpu().double()[ok], bad.cpu()[ok], reduction="none")
    assert float((l[ok].double() - ref).abs().max()) < 1e-5
    # repeated calls: bit-identical losses and gradients, every reduction and target kind
    big = _logits(300, 17, 3).to(DEV)
    for tgt in (_targets(300, 17, "index", 3).to(DEV), _targets(300, 17, "prob", 3).to(DEV)):
        for red in ("none", "sum", "mean"):
            outs = []
            for _ in range(2):
                zz = big.clone().requires_grad_(True)
                loss = CrossEntropyLoss(reduction=red)(zz, tgt)
                loss.backward(torch.ones_like(loss))
                outs.append((loss.detach().clone(), zz.grad.clone()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), red


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the sweep's bookkeeping against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _restate(raw_losses, acc, smooth_f, diverge_th, num_iter):
    """torch-lr-finder's range_test bookkeeping: fp32 `total += loss / acc`, then fp64 smoothing / best / stop."""
    hist, best, stop = [], None, None
    for i in range(num_iter):
        total = None
        for a in range(acc):
            l = np.float32(raw_losses[i * acc + a]) / np.float32(acc)
            total = l if total is None else np.float32(total + l)
        raw = float(total)
        if i == 0:
            best = raw
            s = raw
        else:
            s = smooth_f * raw + (1 - smooth_f) * hist[-1] if smooth_f > 0 else raw
            if s < best:
                best = s
        hist.append(s)
        if s > diverge_th * best:
            stop = i
            break
    return hist, best, stop


def _device_sweep(raw_losses, acc, smooth_f, diverge_th, num_iter):
    from mmnn_sts_amd import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    state = torch.empty((L.mmnn_lr_range_state_bytes(num_iter),), dtype=torch.uint8, device=DEV)
    _lib.check(L.mmnn_lr_range_init(state.data_ptr(), num_iter, st), "init")
    losses = torch.tensor(np.asarray(raw_losses, dtype=np.float32), device=DEV)
    for i in range(num_iter):                     # every iteration enqueued, the ones after a stop included: they must change nothing
        for a in range(acc):
            _lib.check(L.mmnn_lr_range_accumulate(state.data_ptr(), losses[i * acc + a:].data_ptr(), float(acc), int(a == 0), st), "acc")
        _lib.check(L.mmnn_lr_range_update(state.data_ptr(), i, smooth_f, 1 - smooth_f, float(diverge_th), st), "update")
    host = state.cpu()
    ints = host[:24].view(torch.int32)
    live, stop, done, n = (int(ints[k]) for k in (1, 2, 3, 4))
    best = float(host[24:32].view(torch.float64)[0])
    hist = host[40:].view(torch.float64).numpy()
    return live, (stop if stop >= 0 else None), done, n, best, hist


def _raw(case, num_iter, acc):
    m = num_iter * acc
    i = np.arange(m, dtype=np.float64)
    if case == "monotone":
        return list(2.5 - 1.5 * i / m)
    if case == "blowup":                          # a drop, then exponential growth
        return list(np.where(i < 0.5 * m, 2.0 - 1.4 * i / m, 1.3 * np.exp(0.35 * (i - 0.5 * m))))
    if case == "stop1":
        return [1.25] * acc + [1250.0] * (m - acc)
    if case == "nan5":
        v = list(2.0 - 0.01 * i)
        for a in range(acc):
            v[5 * acc + a] = float("nan")
        return v
    raise ValueError(case)


@pytest.mark.parametrize("case,smooth_f,acc", [("monotone", 0.05, 1), ("blowup", 0.05, 1), ("stop1", 0.05, 1), ("nan5", 0.05, 1),
                                                ("blowup", 0.0, 1), ("blowup", 0.05, 3), ("monotone", 0.0, 3)])
def test_sweep_state_matches_restatement(case, smooth_f, acc):
    num_iter, th = 40, 5
    raw = _raw(case, num_iter, acc)
    hist, best, stop = _restate(raw, acc, smooth_f, th, num_iter)
    live, dstop, done, n, dbest, dhist = _device_sweep(raw, acc, smooth_f, th, num_iter)
    print(f"{case} smooth_f={smooth_f} acc={acc}: stop {stop} best {best!r}")
    if case in ("blowup", "stop1"):
        assert stop is not None                   # the case is built to stop
    if case == "stop1":
        assert stop == 1
    if case in ("monotone", "nan5"):
        assert stop is None
    assert n == num_iter and done == len(hist) and dstop == stop and live == (0 if stop is not None else 1)
    np.testing.assert_array_equal(dhist[:done], np.asarray(hist))            # bit for bit (NaN where the restatement has NaN)
    assert (dhist[done:] == 0).all()                                          # nothing written after the stop
    assert dbest == best


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. SGD with the learning rate in device memory
# ---------------------------------------------------------------------------------------------------------------------------------
def _refs(ps, gs, offs, first):
    from mmnn_sts_amd import _lib
    refs = (_lib.TensorRef * len(ps))()
    for r, p, g, o in zip(refs, ps, gs, offs):
        r.param, r.grad, r.count, r.flat_offset, r.first_step = p.data_ptr(), g.data_ptr(), p.numel(), o, int(first)
    return refs


@pytest.mark.parametrize("nesterov", [0, 1])
def test_sgd_device_lr_bit_identical(nesterov):
    from mmnn_sts_amd import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=DEV).manual_seed(11 + nesterov)
    n = 1_000_003
    mom, wd = 0.9, 1e-4
    lrs = [0.0123, 3.7e-3, 0.51]
    base = torch.randn((n + 1,), generator=g, device=DEV)
    shapes = [(3, 1024), (3,), (17,), (5, 7)]
    offs = [0]
    for s in shapes[:-1]:
        offs.append(offs[-1] + (math.prod(s) + 3) // 4 * 4)
    total = offs[-1] + (math.prod(shapes[-1]) + 3) // 4 * 4
    small = [torch.randn(s, generator=g, device=DEV) for s in shapes]
    # flat: an aligned buffer and an unaligned view (the scalar path); small: the multi-tensor launch
    sets = {}
    for tag in ("host", "dev"):
        sets[tag] = dict(flat=base[:n].clone(), odd=base.clone()[1:], buf=torch.empty(n, device=DEV), buf_odd=torch.empty(n + 1, device=DEV)[1:],
                         small=[t.clone() for t in small], sbuf=torch.zeros(total, device=DEV))
    lr_dev = torch.tensor(lrs, dtype=torch.float32, device=DEV)
    live = torch.ones((1,), dtype=torch.int32, device=DEV)
    for step in range(3):
        grad = torch.randn((n,), generator=g, device=DEV)
        sgr = [torch.randn(s, generator=g, device=DEV) for s in shapes]
        first = int(step == 0)
        for tag in ("host", "dev"):
            s = sets[tag]
            for p, b in ((s["flat"], s["buf"]), (s["odd"], s["buf_odd"])):
                if tag == "host":
                    _lib.check(L.mmnn_sgd_step(p.data_ptr(), grad.data_ptr(), b.data_ptr(), n, lrs[step], mom, wd, nesterov, first, st), "sgd")
                else:
                    _lib.check(L.mmnn_sgd_step_dev(p.data_ptr(), grad.data_ptr(), b.data_ptr(), n, lr_dev[step:].data_ptr(), live.data_ptr(),
                                                   mom, wd, nesterov, first, st), "sgd_dev")
            refs = _refs(s["small"], sgr, offs, first)
            if tag == "host":
                _lib.check(L.mmnn_sgd_step_multi(refs, len(shapes), s["sbuf"].data_ptr(), lrs[step], mom, wd, nesterov, st), "multi")
            else:
                _lib.check(L.mmnn_sgd_step_multi_dev(refs, len(shapes), s["sbuf"].data_ptr(), lr_dev[step:].data_ptr(), live.data_ptr(), mom, wd,
                                                     nesterov, st), "multi_dev")
        h, d = sets["host"], sets["dev"]
        for k in ("flat", "odd", "buf", "buf_odd", "sbuf"):
            assert torch.equal(h[k], d[k]), (step, k)
        for a, b in zip(h["small"], d["small"]):
            assert torch.equal(a, b), step
    assert not torch.equal(sets["dev"]["flat"], base[:n])          # the steps did move the parameters

    # live == 0: nothing moves, even with inf / NaN gradients
    s = sets["dev"]
    before = {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in s.items()}
    live.zero_()
    grad = torch.full((n,), float("inf"), device=DEV)
    grad[::2] = float("nan")
    sgr = [torch.full(sh, float("nan"), device=DEV) for sh in shapes]
    for p, b in ((s["flat"], s["buf"]), (s["odd"], s["buf_odd"])):
        _lib.check(L.mmnn_sgd_step_dev(p.data_ptr(), grad.data_ptr(), b.data_ptr(), n, lr_dev.data_ptr(), live.data_ptr(), mom, wd, nesterov, 0, st),
                   "sgd_dev")
    _lib.check(L.mmnn_sgd_step_multi_dev(_refs(s["small"], sgr, offs, 0), len(shapes), s["sbuf"].data_ptr(), lr_dev.data_ptr(), live.data_ptr(),
                                         mom, wd, nesterov, st), "multi_dev")
    for k in ("flat", "odd", "buf", "buf_odd", "sbuf"):
        assert torch.equal(s[k], before[k]), k
    for a, b in zip(s["small"], before["small"]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. LRFinder.range_test against a host-driven loop, bit for bit; reset()
# ---------------------------------------------------------------------------------------------------------------------------------
NUM_ITER = 40


def _small_model():
    from mmnn_sts_amd.models.densenet import densenet121
    return densenet121(spatial_dims=3, in_channels=1, out_channels=3, block_config=(2, 2))


def _setup():
    torch.manual_seed(1234)
    sd0 = {k: v.clone() for k, v in _small_model().state_dict().items()}
    g = torch.Generator().manual_seed(77)
    images = torch.randn((6, 1, 32, 32, 32), generator=g)
    events = (torch.rand((6, 3), generator=g) < 0.6).float()
    batches = [(images[i:i + 2].clone().pin_memory(), events[i:i + 2].clone().pin_memory()) for i in range(0, 6, 2)]   # 3 batches: restarts
    return sd0, batches


def _fresh(sd0):
    from mmnn_sts_amd.optim import FusedSGD
    m = _small_model()
    m.load_state_dict(sd0)
    m = m.to(DEV)
    return m, FusedSGD(m, 1e-7, momentum=0.9, nesterov=True, weight_decay=1e-4)


def _host_loop(model, opt, batches, num_iter, end_lr=100, smooth_f=0.05, diverge_th=5):
    """torch-lr-finder's loop with `.item()` every iteration and the group lr set to the fp32-rounded table value."""
    from mmnn_sts_amd.losses.losses import CrossEntropyLoss
    from mmnn_sts_amd.utils.find_lr import lr_schedule
    crit = CrossEntropyLoss()
    lrs = lr_schedule(float(opt.param_groups[0]["lr"]), end_lr, num_iter)
    model.train()
    hist = {"lr": [], "loss": []}
    best, stop = None, None
    it = iter(batches)
    for i in range(num_iter):
        opt.zero_grad()
        try:
            x, y = next(it)
        except StopIteration:
            it = iter(batches)
            x, y = next(it)
        loss = crit(model(x.to(DEV)), y.to(DEV))
        loss.backward()
        opt.param_groups[0]["lr"] = float(np.float32(lrs[i]))
        opt.step()
        raw = loss.item()
        hist["lr"].append(lrs[i])
        if i == 0:
            best = raw
            s = raw
        else:
            s = smooth_f * raw + (1 - smooth_f) * hist["loss"][-1] if smooth_f > 0 else raw
            if s < best:
                best = s
        hist["loss"].append(s)
        if s > diverge_th * best:
            stop = i
            break
    return hist, best, stop


def _opt_state(opt):
    st = opt.snapshot_state()
    return {"bufs": {k: v.cpu() for k, v in st["bufs"].items()}, "rest": None if st["rest_buf"] is None else st["rest_buf"].cpu(),
            "started": st["rest_started"], "groups": st["param_groups"]}


def test_range_test_matches_host_loop_and_reset_restores():
    from mmnn_sts_amd.losses.losses import CrossEntropyLoss
    from mmnn_sts_amd.utils.find_lr import LRFinder
    sd0, batches = _setup()
    ma, oa = _fresh(sd0)
    opt0 = _opt_state(oa)
    finder = LRFinder(ma, oa, CrossEntropyLoss(), device=DEV)
    finder.range_test(batches, end_lr=100, num_iter=NUM_ITER)
    mb, ob = _fresh(sd0)
    hist, best, stop = _host_loop(mb, ob, batches, NUM_ITER)
    print(f"range test: stop {stop}, {len(hist['loss'])} iterations recorded, {finder.iters_enqueued} enqueued, best {best!r}")
    assert finder.history["lr"] == hist["lr"]
    assert finder.history["loss"] == hist["loss"]
    assert finder.best_loss == best and finder.stop_iter == stop
    assert finder.iters_done == len(hist["loss"])
    if stop is not None:
        assert finder.iters_enqueued <= stop + 1 + 2 * 10                    # default max_ahead = 2 * poll_every
    sa, sb = ma.state_dict(), mb.state_dict()
    params = {k for k, _ in ma.named_parameters()}
    for k in sa:
        if k in params or stop is None:
            assert torch.equal(sa[k], sb[k]), k
    a, b = _opt_state(oa), _opt_state(ob)
    assert len(a["bufs"]) == len(b["bufs"]) == 1                          # keyed by the backbone object: one per model
    assert torch.equal(next(iter(a["bufs"].values())), next(iter(b["bufs"].values())))
    assert torch.equal(a["rest"], b["rest"]) and a["started"] == b["started"]

    finder.reset()
    sr = ma.state_dict()
    for k, v in sd0.items():
        assert torch.equal(sr[k].cpu(), v), k
    r = _opt_state(oa)
    assert r["bufs"] == {} and opt0["bufs"] == {} and r["rest"] is None and opt0["rest"] is None
    assert r["started"] == opt0["started"] and r["groups"] == opt0["groups"]
    mc, _ = _fresh(sd0)
    x = batches[0][0].to(DEV)
    with torch.no_grad():
        ya = ma.eval()(x)
        yc = mc.eval()(x)
    assert torch.equal(ya, yc)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. no host waits inside the sweep
# ---------------------------------------------------------------------------------------------------------------------------------
def _count_waits(monkeypatch):
    calls = []

    def wrap(owner, name, cuda_only):
        orig = getattr(owner, name)

        def f(*a, **k):
            if not cuda_only or (a and torch.is_tensor(a[0]) and a[0].is_cuda):
                calls.append(name)
            return orig(*a, **k)
        monkeypatch.setattr(owner, name, f)

    wrap(torch.cuda, "synchronize", False)
    wrap(torch.cuda.Stream, "synchronize", False)
    wrap(torch.cuda.Event, "synchronize", False)
    for name in ("item", "cpu", "tolist", "numpy"):
        wrap(torch.Tensor, name, True)
    orig_to = torch.Tensor.to

    def to(self, *a, **k):
        if self.is_cuda and not k.get("non_blocking", False):
            dst = k.get("device", a[0] if a else None)
            if (isinstance(dst, str) and dst.startswith("cpu")) or (isinstance(dst, torch.device) and dst.type == "cpu"):
                calls.append("to")
        return orig_to(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "to", to)
    return calls


@pytest.mark.parametrize("max_ahead", [None, "default"])
def test_range_test_has_no_host_waits(monkeypatch, max_ahead):
    from mmnn_sts_amd.losses.losses import CrossEntropyLoss
    from mmnn_sts_amd.utils.find_lr import LRFinder
    sd0, batches = _setup()
    m, o = _fresh(sd0)
    finder = LRFinder(m, o, CrossEntropyLoss(), device=DEV)
    torch.cuda.synchronize()
    calls = _count_waits(monkeypatch)
    finder.range_test(batches, end_lr=100, num_iter=NUM_ITER, max_ahead=max_ahead)
    monkeypatch.undo()
    print(f"max_ahead={max_ahead}: {len(calls)} host waits {calls}, {finder.iters_enqueued} iterations enqueued, stop {finder.stop_iter}")
    limit = 1 if max_ahead is None else 1 + math.ceil(NUM_ITER / 10)
    assert len(calls) <= limit, calls
    assert finder.iters_done >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. main.py --lr_finder
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_lr_finder(tmp_path):
    """Full DenseNet121, 100 iterations: lr_finder.csv (lr column = the schedule), the logged suggestion, the uid split, the graph."""
    from mmnn_sts_amd.utils.find_lr import lr_schedule, split_uids, suggest_lr
    log = run_main(["--images", "--classification", "--lr_finder", "--synthetic_patients", "10", "--synthetic_size", "64"], tmp_path, limit_s=900)
    lines = (tmp_path / "lr_finder.csv").read_text().splitlines()
    assert lines[0] == "lr,loss"
    rows = [tuple(float(v) for v in l.split(",")) for l in lines[1:]]
    assert 1 <= len(rows) <= 100
    sched = lr_schedule(1e-7, 100, 100)
    assert [lr for lr, _ in rows] == sched[:len(rows)]
    s = suggest_lr({"lr": [lr for lr, _ in rows], "loss": [l for _, l in rows]})
    print(f"CLI: {len(rows)} rows, suggestion {s}")
    expected = f"Suggested LR: {s:.2E}" if s is not None else "Suggested LR: none"
    assert expected in log, log[-2000:]
    tr, va = split_uids(range(10), 42)
    assert (tmp_path / "train_uids.txt").read_text() == "\n".join(str(u) for u in tr)
    assert (tmp_path / "val_uids.txt").read_text() == "\n".join(str(u) for u in va)
    assert "Training count = 8 Validation count = 2" in log
    assert (tmp_path / "lr_finder.png").stat().st_size > 0
