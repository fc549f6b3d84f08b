#!/usr/bin/env python
"""Time of the texture classes (GLRLM, GLDM, NGTDM: mmnn_sts_amd/radiomics.py, csrc/radiomics_texture.hip) on the workload of
tools/radiomics_time.py: a 512 x 512 x 48 int16 scan (slope 0.25, inter -12.5), the same ellipsoid ROI, bin_width 25, max_bins 256.

    python tools/radiomics_texture_time.py [--steps 20] [--warmup 5] [--repeats 3] [--json profiles/radiomics_texture_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone):
    extract_us / extract_rotating_us               `mmnn_radiomics` alone, one buffer set reused / 24 sets in turn: the figure of
                                                   profiles/radiomics_time.json measured again in this run
    extract_texture_us / extract_texture_rotating_us   `mmnn_radiomics` + `mmnn_radiomics_texture`, the same two ways
    kernels_us             the per-kernel split of one pair of calls (torch.profiler, device time per kernel name, averaged over the calls)
against two yardsticks taken in the same run:
    sweep_floor_us         one read of the 2-byte bin volume per sweep (13 run-length directions + 1 neighbourhood sweep) at
                           copy_TBs, the rate a device-to-device copy of 256 MiB reaches here (bytes read + written over its time)
    numpy_restatement_ms   tests/_radiomics_texture_ref.py: the four tables and the 35 features from the same bin volume, on the host
No target was set in advance: the capability is new."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import radiomics  # noqa: E402
from mmnn_sts_amd.data import ingest  # noqa: E402
from tools.radiomics_time import BIN_WIDTH, MAX_BINS, ROTATING, SHAPE, copy_tbs, ellipsoid, enqueuer, kernel_split, queued_us  # noqa: E402

SWEEPS = 13 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "radiomics_texture_time.json"))
    ap.add_argument("--no_host", action="store_true", help="skip the numpy restatement (it takes the longest)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(100, 3000, SHAPE, dtype=np.int16)
    mask = ellipsoid()
    dev = torch.device("cuda", 0)
    s, m = ingest.upload(scan, dev, 0.25, -12.5), ingest.upload(mask, dev)
    sets = [radiomics.extract(s, m, dev, BIN_WIDTH, MAX_BINS, classes=radiomics.TEXTURE_CLASSES) for _ in range(ROTATING)]
    torch.cuda.synchronize()
    fields = radiomics.unpack_block(sets[0].block.cpu().numpy())
    assert not (fields["empty"] or fields["nonfinite"] or fields["overflow"]), fields
    for r in sets[1:]:
        assert all(torch.equal(getattr(sets[0], k), getattr(r, k)) for k in ("block", "texture", "glrlm", "gldm", "ngtdm_n", "ngtdm_s")), "two calls differ"
    call = enqueuer(s, m)
    turn = [0]

    def first(r):
        call(r, "first")

    def both(r):
        call(r, "first", "texture")

    def rotate(fn):
        def go():
            turn[0] = (turn[0] + 1) % ROTATING
            fn(sets[turn[0]])
        return go

    named = (("extract_us", lambda: first(sets[0])), ("extract_rotating_us", rotate(first)),
             ("extract_texture_us", lambda: both(sets[0])), ("extract_texture_rotating_us", rotate(both)))
    for _, fn in named:
        for _ in range(a.warmup):
            fn()
    runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]          # the variants alternate inside a repeat
    times = {name: round(float(np.median([r[name] for r in runs])), 1) for name, _ in named}
    spread = {name: [round(min(r[name] for r in runs), 1), round(max(r[name] for r in runs), 1)] for name, _ in named}
    tbs = float(np.median([copy_tbs(a.steps) for _ in range(a.repeats)]))
    kernels = kernel_split(lambda: both(sets[0]))
    host_ms = None
    if not a.no_host:
        from tests import _radiomics_ref as R
        from tests import _radiomics_texture_ref as T
        ref = R.restate(scan, mask, BIN_WIDTH, MAX_BINS, (0.25, -12.5))
        B, ng = ref["bins"], ref["n_bins"]
        t = time.perf_counter()
        glrlm = T.count_glrlm(B, MAX_BINS)
        gldm, ngn, ngs = T.count_neighbourhood(B, MAX_BINS)
        for d in range(13):
            T.matrix_features(glrlm[d, :ng], ref["n"])
        T.matrix_features(gldm[:ng], ref["n"])
        T.ngtdm_features(ngn[:ng], ngs[:ng])
        host_ms = round((time.perf_counter() - t) * 1e3, 1)
        r = sets[0]
        got = [getattr(r, k).cpu().numpy().astype(np.int64) for k in ("glrlm", "gldm", "ngtdm_n", "ngtdm_s")]
        assert all(np.array_equal(g, w) for g, w in zip(got, (glrlm, gldm, ngn, ngs))), "device and restatement differ"
    sweep_bytes = SWEEPS * scan.size * 2
    floor = sweep_bytes / (tbs * 1e12) * 1e6
    texture = round(times["extract_texture_us"] - times["extract_us"], 1)
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "roi_voxels": fields["n"], "n_bins": fields["n_bins"],
           "bin_width": BIN_WIDTH, "max_bins": MAX_BINS, **times, "texture_us": texture, "min_max_over_repeats": spread, "kernels_us": kernels,
           "copy_TBs": round(tbs, 2), "sweeps": SWEEPS, "sweep_MB": round(sweep_bytes / 1e6, 2), "sweep_floor_us": round(floor, 1),
           "texture_over_sweep_floor": round(texture / floor, 1), "numpy_restatement_ms": host_ms,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0),
           "restatement_over_texture": None if host_ms is None else round(host_ms * 1e3 / texture, 1)}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
