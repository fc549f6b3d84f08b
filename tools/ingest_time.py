#!/usr/bin/env python
"""Time of the scan ingest (mmnn_sts_amd/data/ingest.py, csrc/ingest.hip) per volume and per 2 x (T1, T2) batch, with HIP events after
warm-up and the calls queued back to back behind a spin kernel (device time alone), beside the host's share per volume: gunzip + parse
of the two .nii.gz files and the pinned upload.

    python tools/ingest_time.py [--steps 50] [--warmup 10] [--case NAME] [--json out.json] [--kernel_stats kernel_stats.csv]

Cases: 512 x 512 x 48 int16 scan + uint8 mask with a 320 x 310 x 39 box; 256 x 256 x 40 with the mask covering everything.  Bytes are the
algorithmic HBM traffic computed from the shapes -- pass A reads every scan and mask byte once, pass C reads the kept box once, 1 MB is
written -- priced against the 6.29 TB/s measured HBM ceiling of the MI355X.  Per-pass times come from a rocprofv3 run of this tool on
ONE case (`rocprofv3 --kernel-trace --stats -- python tools/ingest_time.py --case NAME`); pass its kernel_stats.csv back with
`--kernel_stats` to have each pass's time and its share of the byte floor added to the JSON."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd.data import ingest, nifti  # noqa: E402

HBM_TBS = 6.29
CASES = {
    "512x512x48_box320x310x39": ((512, 512, 48), ((96, 101, 4), (416, 411, 43))),
    "256x256x40_full": ((256, 256, 40), ((0, 0, 0), (256, 256, 40))),
}
PASS_OF_KERNEL = {"ingest_flags_kernel": "pass_a_flags", "ingest_scan_kernel": "pass_b_scan", "ingest_area_kernel": "pass_c_area"}


def make_volume(shape, box, seed):
    rng = np.random.default_rng(seed)
    scan = rng.integers(1, 3000, shape, dtype=np.int16)
    mask = np.zeros(shape, dtype=np.uint8)
    (x0, y0, z0), (x1, y1, z1) = box
    mask[x0:x1, y0:y1, z0:z1] = 1
    return np.asfortranarray(scan), np.asfortranarray(mask)


def pass_bytes(shape, box):
    voxels = int(np.prod(shape))
    kept = int(np.prod([b - a for a, b in zip(*box)]))
    return {"pass_a_flags": voxels * 3, "pass_c_area": kept * 3 + 4 * 64 ** 3, "pass_b_scan": 8 * sum(shape)}


def host_times(scan, mask, repeats=3):
    """ms per volume: gunzip + parse of scan and mask, and the pinned upload of both (events around the copies)."""
    with tempfile.TemporaryDirectory() as d:
        ps, pm = nifti.write(os.path.join(d, "scan.nii.gz"), scan, 0.25, -12.5), nifti.write(os.path.join(d, "mask.nii.gz"), mask)
        gz = []
        for _ in range(repeats):
            t = time.perf_counter()
            a, b = nifti.read(ps), nifti.read(pm)
            gz.append((time.perf_counter() - t) * 1e3)
        file_mb = (os.path.getsize(ps) + os.path.getsize(pm)) / 1e6
    up_host, up_dev = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        keep = (ingest.upload(a, "cuda"), ingest.upload(b, "cuda"))
        e1.record()
        torch.cuda.synchronize()
        up_host.append((time.perf_counter() - t) * 1e3)
        up_dev.append(e0.elapsed_time(e1))
        del keep
    return {"gunzip_parse_ms": round(min(gz), 2), "upload_ms": round(min(up_host), 2), "upload_copy_ms": round(min(up_dev), 3), "gz_file_MB": round(file_mb, 2)}


def queued_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def time_case(name, steps, warmup):
    shape, box = CASES[name]
    host = [make_volume(shape, box, s) for s in range(4)]
    vols = [(ingest.upload(s, "cuda", 0.25, -12.5), ingest.upload(m, "cuda")) for s, m in host]
    batch = torch.empty((2, 2, 64, 64, 64), device="cuda")
    ext = torch.empty((2, 2, 3), dtype=torch.int32, device="cuda")
    ws = torch.empty(ingest.workspace_bytes(*shape), dtype=torch.uint8, device="cuda")

    def one():
        ingest.ingest_volume(vols[0][0], vols[0][1], batch[0, 0], ext[0, 0], ws)

    def four():
        for i, (s, m) in enumerate(vols):
            ingest.ingest_volume(s, m, batch[i // 2, i % 2], ext[i // 2, i % 2], ws)

    for _ in range(warmup):
        four()
    torch.cuda.synchronize()
    want = [b - a for a, b in zip(*box)]
    assert ext.cpu().reshape(-1, 3).tolist() == [want] * 4, ext
    vol_us, batch_us = queued_us(one, steps), queued_us(four, steps)
    pb = pass_bytes(shape, box)
    total = sum(pb.values())
    floor_us = total / (HBM_TBS * 1e12) * 1e6
    res = {"device_us_per_volume": round(vol_us, 1), "device_us_per_batch": round(batch_us, 1), "MB_per_volume": round(total / 1e6, 2),
           "hbm_floor_us_per_volume": round(floor_us, 2), "TBps": round(total / (vol_us * 1e-6) / 1e12, 3),
           "share_of_hbm_ceiling": round(total / (vol_us * 1e-6) / 1e12 / HBM_TBS, 3), "pass_MB": {k: round(v / 1e6, 3) for k, v in pb.items()}}
    res["host_per_volume"] = host_times(*host[0])
    return res


def add_kernel_stats(res, path):
    """Per-pass mean time from a rocprofv3 kernel_stats.csv of a ONE-case run, and its share of that pass's byte floor."""
    tot = {}
    for r in csv.DictReader(open(path)):
        for kern, name in PASS_OF_KERNEL.items():
            if kern in r["Name"]:
                ns, calls = tot.get(name, (0.0, 0))
                tot[name] = (ns + float(r["TotalDurationNs"]), calls + int(r["Calls"]))
    out = {name: ns / calls / 1e3 for name, (ns, calls) in tot.items()}
    for name, us in out.items():
        b = res["pass_MB"][name] * 1e6
        res.setdefault("pass_us", {})[name] = round(us, 2)
        res.setdefault("pass_share_of_hbm_ceiling", {})[name] = round(b / (us * 1e-6) / 1e12 / HBM_TBS, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--case", type=str, default=None, choices=sorted(CASES))
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--kernel_stats", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {}
    for name in ([a.case] if a.case else list(CASES)):
        res[name] = time_case(name, a.steps, a.warmup)
        if a.kernel_stats and a.case:
            add_kernel_stats(res[name], a.kernel_stats)
        print(json.dumps({"case": name, **res[name]}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
