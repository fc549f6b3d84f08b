#!/usr/bin/env python
"""What the volume cache (mmnn_sts_amd/data/cache.py, csrc/gather.hip) costs and saves, in one run:

  gather      device time of the two `mmnn_gather_rows` calls that assemble a (2, 2, 64^3) and a (2, 2, 128^3) batch out of a table of 256
              slots, with HIP events after warm-up and the calls queued back to back behind a spin kernel.  The slots walk the table
              (512 MB at 64^3, 4 GB at 128^3: beyond the last-level cache) and the destinations rotate, so no call finds its rows or its
              batch where the one before left them.  Priced against the read + write of the batch at the rate a device-to-device
              `copy_` of the same rows reaches in the same run, queued the same way.
  loader      host wall-clock per patient of a loader pass (batch 2, no workers, `IngestCollate(cache=)` over `CachedByUIDs`) over a
              `synth_nifti` tree of 512 x 512 x 48 scans: the first pass reads the files, the second finds every patient in the cache.
  end_to_end  seconds of `main.py --images --preop --survival --blend --epochs 3` on that tree with and without `--cache_volumes`.

`--steps` beyond a few hundred outrun the spin kernel: a 64^3 gather is shorter on the device than its enqueue on the host, and the
window then measures the host.

    python tools/cache_time.py [--steps 200] [--warmup 20] [--patients 4] [--parts gather loader end_to_end] [--json profiles/cache_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mmnn_sts_amd.data import cache as C  # noqa: E402
from mmnn_sts_amd.data import ingest, synth_nifti  # noqa: E402
from mmnn_sts_amd.data.ImageDatasets import ImageDataset, T1T2SurvivalDataset  # noqa: E402

SLOTS, BATCH, CHANNELS, ROTATE = 256, 2, 2, 8
PARTS = ("gather", "loader", "end_to_end")
INGEST_US_PER_BATCH = 306.0                  # what the gather of a (2, 2, 64^3) batch replaces


def queued_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    a.record()
    for k in range(steps):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def time_gather(size, steps, warmup):
    cache = C.VolumeCache("cuda", CHANNELS, size, SLOTS)
    cache.planes.normal_()
    cache.extents.fill_(size)
    outs = [(torch.empty((BATCH, CHANNELS, size, size, size), device="cuda"), torch.empty((BATCH, CHANNELS, 3), dtype=torch.int32, device="cuda"))
            for _ in range(ROTATE)]
    pairs = [[(37 * k) % SLOTS, (37 * k + 101) % SLOTS] for k in range(SLOTS)]       # two rows far apart, another pair every call

    def gather(k):
        cache.gather(pairs[k % SLOTS], *outs[k % ROTATE])

    def planes_only(k):
        C.gather_rows(cache.planes, pairs[k % SLOTS], outs[k % ROTATE][0])

    def copy(k):                                                                      # the same bytes, rows adjacent, by the runtime's copy
        s = (37 * k) % (SLOTS - 1)
        outs[k % ROTATE][0].copy_(cache.planes[s:s + BATCH])

    for fn in (gather, planes_only, copy):
        for k in range(warmup):
            fn(k)
    torch.cuda.synchronize()
    want = cache.planes[pairs[(steps - 1) % SLOTS]]
    gather(steps - 1)
    assert torch.equal(outs[(steps - 1) % ROTATE][0], want)
    moved = 2 * BATCH * CHANNELS * size ** 3 * 4                                      # read + write of the planes
    gather_us, planes_us, copy_us = (min(queued_us(fn, steps) for _ in range(3)) for fn in (gather, planes_only, copy))
    rate = moved / (copy_us * 1e-6) / 1e12
    return {"batch": [BATCH, CHANNELS, size, size, size], "table_slots": SLOTS, "table_MB": round(SLOTS * C.row_bytes(CHANNELS, size) / 1e6, 1),
            "gather_us_per_batch": round(gather_us, 2), "planes_gather_us": round(planes_us, 2), "extents_gather_us": round(gather_us - planes_us, 2),
            "copy_us_same_bytes": round(copy_us, 2), "copy_rate_TBps": round(rate, 3), "MB_read_plus_written": round(moved / 1e6, 2),
            "planes_gather_TBps": round(moved / (planes_us * 1e-6) / 1e12, 3), "planes_gather_over_copy": round(planes_us / copy_us, 3)}


def time_loader(tree):
    ds = T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])
    cache = C.VolumeCache("cuda", CHANNELS, ingest.SIZE, len(ds))
    collate = ingest.IngestCollate("cuda", cache=cache)
    loader = torch.utils.data.DataLoader(C.CachedByUIDs(ds, ds.uids, cache), batch_size=BATCH, shuffle=False, collate_fn=collate)
    res = {"patients": len(ds), "scan": [512, 512, 48]}
    for name in ("first_pass_files", "second_pass_cache"):
        ImageDataset.files_read = 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in loader:
            pass
        torch.cuda.synchronize()
        res[name] = {"host_ms_per_patient": round((time.perf_counter() - t) * 1e3 / len(ds), 3), "files_read": ImageDataset.files_read,
                     "counters_hits_misses_overflow": list(cache.table.take_counters())}
    assert collate.take_empty() == []
    return res


def time_end_to_end(tree, out):
    args = [sys.executable, os.path.join(ROOT, "main.py"), "--images", "--preop", "--survival", "--blend", "--epochs", "3",
            "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
            "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]
    res = {"command": "main.py --images --preop --survival --blend --epochs 3"}
    for name, extra in (("without_cache_s", []), ("with_cache_volumes_s", ["--cache_volumes"])):
        d = os.path.join(out, name)
        os.makedirs(d)
        t = time.perf_counter()
        r = subprocess.run([*args, *extra, "--output_path", d], cwd=d, capture_output=True, text=True)
        res[name] = round(time.perf_counter() - t, 2)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        if extra:
            res["cache_lines"] = [l for l in (r.stdout + r.stderr).splitlines() if l.startswith("volume cache:")]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--patients", type=int, default=4)
    ap.add_argument("--parts", nargs="+", default=list(PARTS), choices=PARTS)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {}
    if "gather" in a.parts:
        res["gather"] = {f"size_{s}": time_gather(s, a.steps, a.warmup) for s in (64, 128)}
        g64 = res["gather"]["size_64"]["gather_us_per_batch"]
        res["gather"]["replaces_ingest_us_per_batch"] = INGEST_US_PER_BATCH
        res["gather"]["gather_over_ingest_at_64"] = round(g64 / INGEST_US_PER_BATCH, 4)
        print(json.dumps(res), flush=True)
    with tempfile.TemporaryDirectory() as d:
        if "loader" in a.parts or "end_to_end" in a.parts:
            tree = synth_nifti.write_tree(os.path.join(d, "tree"), n_patients=a.patients, seed=7, extent=((512, 512), (512, 512), (48, 48)), val_fraction=0.5)
        if "loader" in a.parts:
            res["loader"] = time_loader(tree)
            print(json.dumps(res["loader"]), flush=True)
        if "end_to_end" in a.parts:
            res["end_to_end"] = dict(time_end_to_end(tree, d), patients=a.patients)
            print(json.dumps(res["end_to_end"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
