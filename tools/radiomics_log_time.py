#!/usr/bin/env python
"""Time of the Laplacian-of-Gaussian filter (mmnn_sts_amd/radiomics.py: log_filter, csrc/radiomics_filter.hip) and of a filtered image's
extraction on the workload of tools/radiomics_time.py: a 512 x 512 x 48 int16 scan (slope 0.25, inter -12.5), the same ellipsoid ROI,
max_bins 256, voxel spacing 0.8 x 0.8 x 5 mm, sigma = 1, 3 and 5 mm.

    python tools/radiomics_log_time.py [--steps 10] [--warmup 3] [--repeats 3] [--json profiles/radiomics_log_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone), per sigma:
    filter_us / filter_rotating_us        `mmnn_log_filter` alone, with one buffer set and with 24 in turn
    extract_us / extract_rotating_us      the filter and `mmnn_radiomics` on its output (first order and GLCM) under the device mask
    kernels_us                            the per-kernel split of one filter call (torch.profiler, device time per kernel name)
against the traffic of the contract -- one read of the scan, one write of `out` -- at the copy rate measured in the same run
(`copy_TBs`: a device-to-device copy of 256 MiB, bytes read plus bytes written over its time):
    contract_floor_us, filter_over_floor
The filter itself moves more: it keeps four fp64 intermediates (`moved_MB`: the scan, 2 x 8 B written and read per voxel twice, `out`).
Each filtered image is binned at the smallest multiple of 25 that keeps its whole range within 200 bins (`bin_width`, `n_bins`).
No target was set in advance: the capability is new."""
import argparse
import ctypes
import dataclasses
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import _lib, radiomics  # noqa: E402
from mmnn_sts_amd.data import ingest  # noqa: E402
from tools.radiomics_time import BIN_WIDTH, MAX_BINS, ROTATING, SHAPE, copy_tbs, ellipsoid, kernel_split, queued_us  # noqa: E402

SPACING = (0.8, 0.8, 5.0)
SIGMAS = (1.0, 3.0, 5.0)
COPY_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "radiomics_log_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(100, 3000, SHAPE, dtype=np.int16)
    mask = ellipsoid()
    dev = torch.device("cuda", 0)
    aff = np.diag(list(SPACING) + [1.0])
    s = dataclasses.replace(ingest.upload(scan, dev, 0.25, -12.5), affine=aff)
    m = dataclasses.replace(ingest.upload(mask, dev), affine=aff)
    n = int(np.prod(SHAPE))
    stream = torch.cuda.current_stream().cuda_stream
    L = _lib.lib()
    tbs = float(np.median([copy_tbs(a.steps) for _ in range(a.repeats)]))
    copy_us = 2 * COPY_BYTES / (tbs * 1e12) * 1e6
    floor_us = (scan.nbytes + n * 4) / (tbs * 1e12) * 1e6
    ws = [torch.empty(L.mmnn_log_filter_workspace_bytes(*SHAPE), dtype=torch.uint8, device=dev) for _ in range(ROTATING)]
    per_sigma = {}
    for sigma in SIGMAS:
        radius, taps, weight = radiomics.log_taps(sigma, SPACING)
        first = radiomics.log_filter(s, sigma, dev, workspace=ws[0])
        again = radiomics.log_filter(s, sigma, dev, workspace=ws[1])
        assert torch.equal(first.data, again.data), "two calls differ"
        f32 = first.data.view(torch.float32)
        span = float(f32.max() - f32.min())
        bw = BIN_WIDTH * max(1, math.ceil(span / (BIN_WIDTH * 200)))
        del again
        sets = [radiomics.extract(first, m, dev, bw, MAX_BINS) for _ in range(ROTATING)]
        outs = [f32] + [torch.empty_like(f32) for _ in range(ROTATING - 1)]
        tp = torch.from_numpy(taps).to(dev)
        torch.cuda.synchronize()
        fields = radiomics.unpack_block(sets[0].block.cpu().numpy())
        assert not (fields["empty"] or fields["nonfinite"] or fields["overflow"]), fields
        fdesc = _lib.LogFilterDesc(*SHAPE, s.datatype, s.slope, s.inter, (ctypes.c_int32 * 3)(*radius.tolist()), (ctypes.c_double * 3)(*weight.tolist()))
        rdesc = _lib.RadiomicsDesc(*SHAPE, 16, m.datatype, 0.0, 0.0, m.slope, m.inter, bw, MAX_BINS)
        turn = [0]

        def filt(k):
            _lib.check(L.mmnn_log_filter(ctypes.byref(fdesc), s.data.data_ptr(), tp.data_ptr(), outs[k].data_ptr(), ws[k].data_ptr(), stream),
                       "mmnn_log_filter")

        def both(k):
            filt(k)
            radiomics.enqueue(sets[k], "first", rdesc, stream, outs[k].data_ptr(), m.data.data_ptr())

        def rotate(fn):
            def step():
                turn[0] = (turn[0] + 1) % ROTATING
                fn(turn[0])
            return step

        named = (("filter_us", lambda: filt(0)), ("filter_rotating_us", rotate(filt)), ("extract_us", lambda: both(0)),
                 ("extract_rotating_us", rotate(both)))
        for _, fn in named:
            for _ in range(a.warmup):
                fn()
        runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]     # the variants alternate inside a repeat
        times = {name: round(float(np.median([q[name] for q in runs])), 1) for name, _ in named}
        spread = {name: [round(min(q[name] for q in runs), 1), round(max(q[name] for q in runs), 1)] for name, _ in named}
        torch.cuda.synchronize()
        assert all(torch.equal(outs[0], o) for o in outs[1:]) and all(torch.equal(sets[0].block, r.block) for r in sets[1:]), "two calls differ"
        kernels = kernel_split(lambda: filt(0))
        per_sigma[str(sigma)] = {"radius": radius.tolist(), "bin_width": bw, "n_bins": fields["n_bins"], **times, "min_max_over_repeats": spread,
                                 "filter_over_floor": round(times["filter_us"] / floor_us, 1), "kernels_us": kernels}
        del sets, outs, first, f32
    res = {"shape": list(SHAPE), "spacing_mm": list(SPACING), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "buffer_sets": ROTATING,
           "copy_MB": COPY_BYTES >> 20, "copy_us": round(copy_us, 1), "copy_TBs": round(tbs, 2),
           "contract_MB": round((scan.nbytes + n * 4) / 1e6, 2), "contract_floor_us": round(floor_us, 1),
           "moved_MB": round((scan.nbytes + n * (16 + 16 + 16 + 16) + n * 4) / 1e6, 1), "workspace_MB": round(ws[0].numel() / 1e6, 1),
           "max_radius": _lib.LOG_FILTER_MAX_RADIUS, "sigma_mm": per_sigma}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
