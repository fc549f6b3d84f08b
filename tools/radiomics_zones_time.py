#!/usr/bin/env python
"""Time of the size-zone class (GLSZM: mmnn_sts_amd/radiomics.py, csrc/radiomics_zones.hip) on the workload of tools/radiomics_time.py:
a 512 x 512 x 48 int16 scan (slope 0.25, inter -12.5), the same ellipsoid ROI, bin_width 25, max_bins 256.

    python tools/radiomics_zones_time.py [--steps 20] [--warmup 5] [--repeats 3] [--json profiles/radiomics_zones_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone):
    extract_texture_us / extract_texture_rotating_us   `mmnn_radiomics` + `mmnn_radiomics_texture`, one buffer set reused / 24 sets in
                                                       turn: the figure of profiles/radiomics_texture_time.json measured again in this run
    extract_all_us / extract_all_rotating_us           the two calls + `mmnn_radiomics_zones`, the same two ways
    kernels_us             the per-kernel split of one triple of calls (torch.profiler, device time per kernel name, averaged over the calls)
against two yardsticks taken in the same run:
    label_floor_us         one read of the 2-byte bin volume plus one write and one read of a 4-byte label volume at copy_TBs, the rate a
                           device-to-device copy of 256 MiB reaches here (bytes read + written over its time)
    restatement_ms         tests/_radiomics_zones_ref.py: scipy.ndimage.label per level, the sizes, the keys and the 16 features from the
                           same bin volume, on the host
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "radiomics_zones_time.json"))
    ap.add_argument("--no_host", action="store_true", help="skip the scipy restatement (it takes the longest)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(100, 3000, SHAPE, dtype=np.int16)
    mask = ellipsoid()
    dev = torch.device("cuda", 0)
    s, m = ingest.upload(scan, dev, 0.25, -12.5), ingest.upload(mask, dev)
    sets = [radiomics.extract(s, m, dev, BIN_WIDTH, MAX_BINS, classes=radiomics.TEXTURE_CLASSES, glszm=True) for _ in range(ROTATING)]
    torch.cuda.synchronize()
    fields = radiomics.unpack_block(sets[0].block.cpu().numpy())
    assert not (fields["empty"] or fields["nonfinite"] or fields["overflow"]), fields
    for r in sets[1:]:
        assert all(torch.equal(getattr(sets[0], k), getattr(r, k)) for k in ("block", "texture", "zones", "labels", "sizes", "levels")), "two calls differ"
    zones = radiomics.unpack_zones(sets[0].zones.cpu().numpy())
    call = enqueuer(s, m)
    turn = [0]

    def two(r):
        call(r, "first", "texture")

    def three(r):
        call(r, "first", "texture", "zones")

    def rotate(fn):
        def go():
            turn[0] = (turn[0] + 1) % ROTATING
            fn(sets[turn[0]])
        return go

    named = (("extract_texture_us", lambda: two(sets[0])), ("extract_texture_rotating_us", rotate(two)),
             ("extract_all_us", lambda: three(sets[0])), ("extract_all_rotating_us", rotate(three)))
    for _, fn in named:
        for _ in range(a.warmup):
            fn()
    runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]          # the variants alternate inside a repeat
    times = {name: round(float(np.median([r[name] for r in runs])), 1) for name, _ in named}
    spread = {name: [round(min(r[name] for r in runs), 1), round(max(r[name] for r in runs), 1)] for name, _ in named}
    tbs = float(np.median([copy_tbs(a.steps) for _ in range(a.repeats)]))
    kernels = kernel_split(lambda: three(sets[0]))
    host_ms = None
    if not a.no_host:
        from tests import _radiomics_ref as R
        from tests import _radiomics_zones_ref as Z
        ref = R.restate(scan, mask, BIN_WIDTH, MAX_BINS, (0.25, -12.5))
        B = ref["bins"].astype(np.int64)
        t = time.perf_counter()
        labels, sizes = Z.label_zones(B)
        I, J, C = Z.zone_keys(B, sizes)
        Z.features(I, J, C, ref["n_bins"], ref["n"])
        host_ms = round((time.perf_counter() - t) * 1e3, 1)
        r = sets[0]
        assert np.array_equal(r.labels.cpu().numpy().astype(np.int64), Z.flat(labels)), "device and restatement differ: labels"
        assert np.array_equal(r.sizes.cpu().numpy().astype(np.int64), Z.flat(sizes)), "device and restatement differ: sizes"
        assert (zones["nz"], zones["n_keys"], zones["max_size"]) == (int(C.sum()), len(C), int(J.max())), "device and restatement differ: integers"
    label_bytes = scan.size * (2 + 4 + 4)
    floor = label_bytes / (tbs * 1e12) * 1e6
    zone_us = round(times["extract_all_us"] - times["extract_texture_us"], 1)
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "roi_voxels": fields["n"], "n_bins": fields["n_bins"],
           "bin_width": BIN_WIDTH, "max_bins": MAX_BINS, "zones": zones["nz"], "distinct_keys": zones["n_keys"], "largest_zone": zones["max_size"],
           "key_bound": round(float(np.sqrt(2.0 * fields["n"] * fields["n_bins"])), 1), **times, "zones_us": zone_us,
           "zones_rotating_us": round(times["extract_all_rotating_us"] - times["extract_texture_rotating_us"], 1),
           "min_max_over_repeats": spread, "kernels_us": kernels, "copy_TBs": round(tbs, 2), "label_MB": round(label_bytes / 1e6, 2),
           "label_floor_us": round(floor, 1), "zones_over_label_floor": round(zone_us / floor, 1), "restatement_ms": host_ms,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0),
           "restatement_over_zones": None if host_ms is None else round(host_ms * 1e3 / zone_us, 1)}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
