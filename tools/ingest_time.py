#!/usr/bin/env python
"""Time of the scan ingest (mmnn_sts_amd/data/ingest.py, csrc/ingest.hip) per volume and per 2 x (T1, T2) batch, with HIP events after
warm-up and the calls queued back to back behind a spin kernel (device time alone), beside the host's share per volume: gunzip + parse
of the two .nii.gz files and the pinned upload.

    python tools/ingest_time.py [--steps 50] [--warmup 10] [--case NAME] [--mask_grid own] [--json out.json] [--kernel_stats kernel_stats.csv]
    python tools/ingest_time.py --maps_to_scan [--json out.json]      # the inverse path alone (`--json` adds its rows to the file's)
    python tools/ingest_time.py --size 64 128 [--json out.json]       # both paths at each output extent S (`--json` adds its rows to the file's)

Cases: 512 x 512 x 48 int16 scan + uint8 mask with a 320 x 310 x 39 box; 256 x 256 x 40 with the mask covering everything.  Bytes are the
algorithmic HBM traffic computed from the shapes -- pass A reads every scan and mask byte once, pass C reads the kept box once, 1 MB is
written -- priced against the 6.29 TB/s measured HBM ceiling of the MI355X.  Per-pass times come from a rocprofv3 run of this tool on
ONE case (`rocprofv3 --kernel-trace --stats -- python tools/ingest_time.py --case NAME`); pass its kernel_stats.csv back with
`--kernel_stats` to have each pass's time and its share of the byte floor added to the JSON.

`--mask_grid own` draws the same box on a mask grid of 3/4 the scan's extents per axis (384 x 384 x 36 for 512 x 512 x 48; the outer
faces of the two grids coincide, so the resampled box is within a voxel of the same-grid one) and runs `mmnn_resample_mask` ahead of the three passes; its bytes are the mask read
once plus x*y*z written.

`--maps_to_scan` times the way back (`ingest.maps_to_scan`, 64^3 maps -> fp32 volumes on the scan's grid) on the first case's scan, with 1
map and with 2, from the workspace one ingest left behind.  Its floor is the bytes WRITTEN (n_maps * x*y*z * 4; the 1 MB map per volume
and the tap tables are read from cache) over the same 6.29 TB/s.

`--size S [S ...]` (1..128) times, in one run and on the first case (or `--case`), the ingest to S^3 planes and the way back from S^3
maps at every S named, under the key `sizes_<case>`: {"size_<S>": {"ingest": ..., "maps_to_scan": ...}}.  Without it S is 64 and the
keys are the ones above."""
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
PASS_OF_KERNEL = {"resample_mask_kernel": "pass_r_resample", "ingest_flags_kernel": "pass_a_flags", "ingest_scan_kernel": "pass_b_scan", "ingest_area_kernel": "pass_c_area"}


def make_volume(shape, box, seed):
    rng = np.random.default_rng(seed)
    scan = rng.integers(1, 3000, shape, dtype=np.int16)
    mask = np.zeros(shape, dtype=np.uint8)
    (x0, y0, z0), (x1, y1, z1) = box
    mask[x0:x1, y0:y1, z0:z1] = 1
    return np.asfortranarray(scan), np.asfortranarray(mask)


def own_grid(shape, box):
    """(mask extents, the box on the mask grid, index map): a grid of 3/4 the extents whose outer faces coincide with the scan's, so
    mask index = 0.75 (i + 0.5) - 0.5.  The box is the case's, scaled and rounded down; the caller reads the kept extents it leaves."""
    own = tuple(-(-3 * n // 4) for n in shape)
    lo, hi = ([int(np.floor(0.75 * v)) for v in b] for b in box)
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = np.diag([0.75] * 3), 0.75 * 0.5 - 0.5
    return own, (tuple(lo), tuple(hi)), T


def pass_bytes(shape, box, own=None, size=ingest.SIZE):
    voxels = int(np.prod(shape))
    kept = int(np.prod([b - a for a, b in zip(*box)]))
    pb = {"pass_a_flags": voxels * 3, "pass_c_area": kept * 3 + 4 * size ** 3, "pass_b_scan": 8 * sum(shape)}
    if own is not None:
        pb["pass_r_resample"] = int(np.prod(own)) + voxels
    return pb


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


def time_case(name, steps, warmup, mask_grid="same", size=ingest.SIZE):
    shape, box = CASES[name]
    host = [make_volume(shape, box, s) for s in range(4)]
    own = None
    if mask_grid == "own":
        own, own_box, T = own_grid(shape, box)
        host = [(s, make_volume(own, own_box, 0)[1]) for s, _ in host]
        resampled = torch.empty(int(np.prod(shape)), dtype=torch.uint8, device="cuda")
    vols = [(ingest.upload(s, "cuda", 0.25, -12.5), ingest.upload(m, "cuda")) for s, m in host]
    batch = torch.empty((2, 2, size, size, size), device="cuda")
    ext = torch.empty((2, 2, 3), dtype=torch.int32, device="cuda")
    ws = torch.empty(ingest.workspace_bytes(*shape), dtype=torch.uint8, device="cuda")

    def volume(i):
        s, m = vols[i]
        if own is not None:       # (one buffer for the resampled mask: the four volumes run in stream order)
            m = ingest.resample_mask(m, shape, T, 0.5, out=resampled)
        ingest.ingest_volume(s, m, batch[i // 2, i % 2], ext[i // 2, i % 2], ws)

    def one():
        volume(0)

    def four():
        for i in range(4):
            volume(i)

    for _ in range(warmup):
        four()
    torch.cuda.synchronize()
    got = ext.cpu().reshape(-1, 3).tolist()
    if own is None:
        assert got == [[b - a for a, b in zip(*box)]] * 4, ext
    else:                         # the kept box in scan voxels, for the byte count of pass C
        assert got == [got[0]] * 4 and min(got[0]) > 0, ext
        box = ((0, 0, 0), tuple(got[0]))
    vol_us, batch_us = queued_us(one, steps), queued_us(four, steps)
    pb = pass_bytes(shape, box, own, size)
    total = sum(pb.values())
    floor_us = total / (HBM_TBS * 1e12) * 1e6
    res = {"device_us_per_volume": round(vol_us, 1), "device_us_per_batch": round(batch_us, 1), "MB_per_volume": round(total / 1e6, 2),
           "hbm_floor_us_per_volume": round(floor_us, 2), "TBps": round(total / (vol_us * 1e-6) / 1e12, 3),
           "share_of_hbm_ceiling": round(total / (vol_us * 1e-6) / 1e12 / HBM_TBS, 3), "pass_MB": {k: round(v / 1e6, 3) for k, v in pb.items()}, "pass_bytes": pb}
    if own is not None:
        res["mask_grid"] = list(own)
        res["resample_us_per_volume"] = round(queued_us(lambda: ingest.resample_mask(vols[0][1], shape, T, 0.5, out=resampled), steps), 1)
    res["host_per_volume"] = host_times(*host[0])
    return res


def time_maps_to_scan(steps, warmup, name="512x512x48_box320x310x39", size=ingest.SIZE):
    shape, box = CASES[name]
    scan, mask = make_volume(shape, box, 0)
    ws = torch.empty(ingest.workspace_bytes(*shape), dtype=torch.uint8, device="cuda")
    ext = ingest.ingest_volume(ingest.upload(scan, "cuda", 0.25, -12.5), ingest.upload(mask, "cuda"), torch.empty((size, size, size), device="cuda"), workspace=ws)
    assert ext.cpu().tolist() == [b - a for a, b in zip(*box)], ext
    scratch = torch.empty(ingest.maps_to_scan_workspace_bytes(*shape), dtype=torch.uint8, device="cuda")
    res = {"scan": list(shape), "kept": ext.cpu().tolist()}
    for n in (1, 2):
        maps = torch.rand((n, size, size, size), device="cuda")
        out = torch.empty((n, *shape[::-1]), device="cuda")
        fn = lambda: ingest.maps_to_scan(maps, shape, ws, out=out, workspace=scratch)
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        us = queued_us(fn, steps)
        written = n * int(np.prod(shape)) * 4
        floor_us = written / (HBM_TBS * 1e12) * 1e6
        res[f"n_maps_{n}"] = {"device_us_per_call": round(us, 1), "MB_written": round(written / 1e6, 2), "hbm_floor_us": round(floor_us, 2),
                              "TBps": round(written / (us * 1e-6) / 1e12, 3), "share_of_hbm_ceiling": round(floor_us / us, 3)}
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
        b = res["pass_bytes"][name]
        res.setdefault("pass_us", {})[name] = round(us, 2)
        res.setdefault("pass_share_of_hbm_ceiling", {})[name] = round(b / (us * 1e-6) / 1e12 / HBM_TBS, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--case", type=str, default=None, choices=sorted(CASES))
    ap.add_argument("--mask_grid", type=str, default="same", choices=("same", "own"), help="own: the mask on a grid of 3/4 the extents, resampled first")
    ap.add_argument("--maps_to_scan", action="store_true", help="time the inverse path (maps_to_scan, 1 and 2 maps) instead of the ingest cases")
    ap.add_argument("--size", type=int, nargs="+", default=None, metavar="S",
                    help="output extents per axis (1..128): time the ingest and the inverse path of one case at each of them instead")
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--kernel_stats", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {}
    if a.size:
        name = a.case or next(iter(CASES))
        rows = res["sizes_" + name] = {}
        for size in a.size:
            rows[f"size_{size}"] = {"ingest": time_case(name, a.steps, a.warmup, a.mask_grid, size),
                                    "maps_to_scan": time_maps_to_scan(a.steps, a.warmup, name, size)}
            print(json.dumps({"case": name, "size": size, **rows[f"size_{size}"]}), flush=True)
        if a.json and os.path.exists(a.json):       # its rows join the file's
            res = {**json.load(open(a.json)), **res}
    elif a.maps_to_scan:
        res["maps_to_scan_512x512x48"] = time_maps_to_scan(a.steps, a.warmup)
        print(json.dumps({"case": "maps_to_scan_512x512x48", **res["maps_to_scan_512x512x48"]}), flush=True)
        if a.json and os.path.exists(a.json):       # its rows join the ingest's
            res = {**json.load(open(a.json)), **res}
    for name in ([] if a.maps_to_scan or a.size else [a.case] if a.case else list(CASES)):
        key = name if a.mask_grid == "same" else name + "_mask_grid_own"
        res[key] = time_case(name, a.steps, a.warmup, a.mask_grid)
        if a.kernel_stats and a.case:
            add_kernel_stats(res[key], a.kernel_stats)
        print(json.dumps({"case": key, **res[key]}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
