#!/usr/bin/env python
"""Time of one radiomics extraction (mmnn_sts_amd/radiomics.py, csrc/radiomics.hip): a 512 x 512 x 48 int16 scan (slope 0.25, inter
-12.5) whose ROI is the ellipsoid of tools/seg_time.py, bin_width 25, max_bins 256.

    python tools/radiomics_time.py [--steps 20] [--warmup 5] [--repeats 3] [--json profiles/radiomics_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone), as in
tools/rtstruct_time.py:
    extract_us             `mmnn_radiomics`, scan and mask on the device, one set of result / hist / glcm / workspace buffers reused
    extract_rotating_us    ... with 24 buffer sets in turn
    kernels                the per-kernel split of one call (torch.profiler, device time per kernel name, averaged over the profiled calls)
against two yardsticks taken in the same run:
    one_read_floor_us      scan + mask read once at the 6.29 TB/s the other timing tools price HBM traffic at
    numpy_restatement_ms   tests/_radiomics_ref.py: restate() of the same volume on the host
No target was set in advance and the capability is new, so there is no parent-commit figure."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import _lib, radiomics  # noqa: E402
from mmnn_sts_amd.data import ingest  # noqa: E402

HBM_TBS = 6.29
SHAPE = (512, 512, 48)
CENTRE, RADIUS = (262.3, 249.6, 23.4), (163.7, 151.2, 10.2)
ROTATING = 24
BIN_WIDTH, MAX_BINS = 25.0, 256


def queued_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def copy_tbs(steps):
    """Device-to-device copy rate, read + written bytes per second, in TB/s."""
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    us = queued_us(lambda: dst.copy_(src), steps)
    return 2 * src.numel() / (us * 1e-6) / 1e12


def kernel_split(fn, calls=3):
    """The per-kernel split of `fn` (torch.profiler, device time per kernel name in us, averaged over `calls` calls), longest first."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        kernels = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            if t:
                kernels[ev.key[:80]] = round(t / calls, 1)
        return dict(sorted(kernels.items(), key=lambda kv: -kv[1]))
    except Exception as e:                                   # the split is an aid; the totals stand without it
        return {"unavailable": repr(e)[:200]}


def enqueuer(s, m, bin_width=BIN_WIDTH):
    """call(result, *stages): the calls of `radiomics.STAGES` named, on the uploaded scan `s` and mask `m`, into the result's buffers."""
    desc = _lib.RadiomicsDesc(*SHAPE, s.datatype, m.datatype, s.slope, s.inter, m.slope, m.inter, bin_width, MAX_BINS)
    stream = torch.cuda.current_stream().cuda_stream

    def call(r, *stages):
        for st in stages:
            radiomics.enqueue(r, st, desc, stream, s.data.data_ptr(), m.data.data_ptr())
    return call


def ellipsoid():
    g = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in SHAPE], indexing="ij", sparse=True)
    return (sum(((v - c) / r) ** 2 for v, c, r in zip(g, CENTRE, RADIUS)) <= 1.0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "radiomics_time.json"))
    ap.add_argument("--no_host", action="store_true", help="skip the numpy restatement (it takes the longest)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(100, 3000, SHAPE, dtype=np.int16)
    mask = ellipsoid()
    dev = torch.device("cuda", 0)
    s, m = ingest.upload(scan, dev, 0.25, -12.5), ingest.upload(mask, dev)
    sets = [radiomics.extract(s, m, dev, BIN_WIDTH, MAX_BINS) for _ in range(ROTATING)]
    torch.cuda.synchronize()
    fields = radiomics.unpack_block(sets[0].block.cpu().numpy())
    assert not (fields["empty"] or fields["nonfinite"] or fields["overflow"]), fields
    assert all(torch.equal(sets[0].block, r.block) and torch.equal(sets[0].glcm, r.glcm) for r in sets[1:]), "two calls differ"
    call = enqueuer(s, m)
    turn = [0]

    def reused():
        call(sets[0], "first")

    def rotating():
        turn[0] = (turn[0] + 1) % ROTATING
        call(sets[turn[0]], "first")

    named = (("extract_us", reused), ("extract_rotating_us", rotating))
    for _, fn in named:
        for _ in range(a.warmup):
            fn()
    runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]
    times = {name: round(float(np.median([r[name] for r in runs])), 1) for name, _ in named}
    spread = {name: [round(min(r[name] for r in runs), 1), round(max(r[name] for r in runs), 1)] for name, _ in named}
    kernels = kernel_split(reused)
    host_ms = None
    if not a.no_host:
        from tests import _radiomics_ref as R
        t = time.perf_counter()
        ref = R.restate(scan, mask, BIN_WIDTH, MAX_BINS, (0.25, -12.5))
        host_ms = round((time.perf_counter() - t) * 1e3, 1)
        glcm = sets[0].glcm.cpu().numpy().astype(np.int64)
        assert ref["n"] == fields["n"] and ref["n_bins"] == fields["n_bins"] and np.array_equal(ref["glcm"], glcm), "device and restatement differ"
        assert np.array_equal(ref["order"].view(np.uint64), fields["order"].view(np.uint64))
    read_bytes = scan.nbytes + mask.nbytes
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "roi_voxels": fields["n"], "n_bins": fields["n_bins"],
           "bin_width": BIN_WIDTH, "max_bins": MAX_BINS, **times, "min_max_over_repeats": spread, "kernels_us": kernels,
           "read_MB": round(read_bytes / 1e6, 2), "one_read_floor_us": round(read_bytes / (HBM_TBS * 1e12) * 1e6, 2),
           "extract_over_one_read": round(times["extract_us"] / (read_bytes / (HBM_TBS * 1e12) * 1e6), 1),
           "numpy_restatement_ms": host_ms, "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0),
           "restatement_over_extract": None if host_ms is None else round(host_ms * 1e3 / times["extract_us"], 1)}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
