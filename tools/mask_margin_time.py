#!/usr/bin/env python
"""Time of the mask margin step (ingest.mask_margin, csrc/mask_margin.hip) per volume, beside what it feeds and what it replaces, in one
run: the 512 x 512 x 48 ellipsoid mask of tools/rtstruct_time.py at 0.8 x 0.8 x 5 mm, widened by 5, 10 and 20 mm in both modes.

    python tools/mask_margin_time.py [--steps 30] [--warmup 5] [--repeats 3] [--json profiles/mask_margin_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone), as in
tools/rtstruct_time.py:
    <mode>_<r>mm_us              `mmnn_mask_margin` alone, mask and workspace on the device, the same 12.6 MB output every call
    <mode>_<r>mm_rotating_us     ... with 24 output buffers in turn
    copy_GBs, contract_traffic_us   the rate of a device-to-device copy of 302 MB measured in this run (bytes read plus bytes written per
                                 second), and the time one read of the mask plus one write of `out` (25.2 MB, the contract's traffic)
                                 takes at that rate.  The step's own passes move more than that: a byte and a double per voxel written
                                 and read again between the passes (226 MB).
    ingest_us, ingest_margin_<r>mm_us   `ingest_volume` of an int16 scan under the mask, without and with `mask_margin_mm` (the margin's
                                 output and workspace are allocated per call, as the path does it)
    extract_us, extract_shell_<r>mm_us   `radiomics.extract` of the default columns alone and with one shell, buffers reused
The host's alternative is reported beside them: scipy.ndimage.distance_transform_edt(sampling=spacing) of the same mask, wall time.
Before anything is timed, every (radius, mode) result of the device is compared with the separable numpy form of the restatement
(tests/_mask_margin_ref.py); a difference ends the run with an error."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mmnn_sts_amd import radiomics  # noqa: E402
from mmnn_sts_amd.data import ingest  # noqa: E402
from tests import _mask_margin_ref as M  # noqa: E402
from dicom_timing import queued_us  # noqa: E402

SHAPE = (512, 512, 48)
SPACING = (0.8, 0.8, 5.0)
CENTRE, RADIUS = (262.3, 249.6, 23.4), (163.7, 151.2, 17.8)       # voxels: the ellipsoid of tools/rtstruct_time.py
RADII = (5.0, 10.0, 20.0)
ROTATING = 24


def ellipsoid():
    g = [((np.arange(n) - c) / r) ** 2 for n, c, r in zip(SHAPE, CENTRE, RADIUS)]
    return ((g[0][:, None, None] + g[1][None, :, None] + g[2][None, None, :]) <= 1.0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="every figure is the median of this many windows of --steps calls")
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "mask_margin_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    voxels = int(np.prod(SHAPE))
    mask = ellipsoid()
    scan = np.random.default_rng(0).integers(1, 3000, SHAPE, dtype=np.int16)
    affine = np.diag([*SPACING, 1.0])
    vol_m = ingest.upload(mask, "cuda")
    vol_m.affine = affine
    vol_s = ingest.upload(scan, "cuda")
    vol_s.affine = affine
    outs = [torch.empty(voxels, dtype=torch.uint8, device="cuda") for _ in range(ROTATING)]
    ws = torch.empty(ingest.mask_margin_workspace_bytes(*SHAPE), dtype=torch.uint8, device="cuda")

    # the check: device against the separable restatement, every radius and mode
    checked = {}
    for r in RADII:
        t = time.perf_counter()
        D = M.separable(mask != 0, SPACING, M.reach(SPACING, r))
        numpy_s = time.perf_counter() - t
        for mode in ("dilate", "shell"):
            want = M.threshold(D, r, mode)[0]
            got = ingest.mask_margin(vol_m, SPACING, r, mode, out=outs[0], workspace=ws).data.cpu().numpy().reshape(SHAPE, order="F")
            if not np.array_equal(got, want):
                raise SystemExit(f"mask_margin {mode} at {r} mm: {int((got != want).sum())} voxels differ from the restatement")
            checked[f"{mode}_{r:g}mm_voxels_set"] = int(want.sum())
        checked[f"numpy_separable_{r:g}mm_s"] = round(numpy_s, 2)
        del D

    from scipy import ndimage
    t = time.perf_counter()
    edt = ndimage.distance_transform_edt(mask == 0, sampling=SPACING)
    scipy_s = time.perf_counter() - t
    for r in RADII:
        assert int((edt <= r).sum()) == checked[f"dilate_{r:g}mm_voxels_set"], "scipy's thresholded EDT disagrees on the set's size"
    del edt

    turn = [0]
    named = []
    for r in RADII:
        for mode in ("dilate", "shell"):
            def one(r=r, mode=mode):
                ingest.mask_margin(vol_m, SPACING, r, mode, out=outs[0], workspace=ws)

            def rotating(r=r, mode=mode):
                turn[0] = (turn[0] + 1) % ROTATING
                ingest.mask_margin(vol_m, SPACING, r, mode, out=outs[turn[0]], workspace=ws)
            named += [(f"{mode}_{r:g}mm_us", one), (f"{mode}_{r:g}mm_rotating_us", rotating)]

    big = torch.empty(ROTATING * voxels // 2, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)
    named.append(("copy_151MB_us", lambda: big2.copy_(big)))

    plane = torch.empty((64, 64, 64), device="cuda")
    ext = torch.empty(3, dtype=torch.int32, device="cuda")
    iws = torch.empty(ingest.workspace_bytes(*SHAPE), dtype=torch.uint8, device="cuda")
    named.append(("ingest_us", lambda: ingest.ingest_volume(vol_s, vol_m, plane, ext, iws)))
    for r in RADII:
        named.append((f"ingest_margin_{r:g}mm_us", lambda r=r: ingest.ingest_volume(vol_s, vol_m, plane, ext, iws, mask_margin_mm=r)))

    base = radiomics.extract(vol_s, vol_m, "cuda")
    named.append(("extract_us", lambda: radiomics.extract(vol_s, vol_m, "cuda", buffers=base)))
    for r in RADII:
        held = radiomics.extract(vol_s, vol_m, "cuda", shell_mm=[r])
        named.append((f"extract_shell_{r:g}mm_us", lambda r=r, held=held: radiomics.extract(vol_s, vol_m, "cuda", shell_mm=[r], buffers=held)))
    torch.cuda.synchronize()
    feats = radiomics.finish(held)
    assert len(feats) == 47 + 41 and all(np.isfinite(v) for k, v in feats.items() if k.startswith("shell-"))

    for _, fn in named:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]
    times = {name: round(float(np.median([r[name] for r in runs])), 1) for name, _ in named}
    spread = {name: [round(min(r[name] for r in runs), 1), round(max(r[name] for r in runs), 1)] for name, _ in named}
    copy_rate = 2 * big.numel() / (times["copy_151MB_us"] * 1e-6)                  # bytes read + bytes written per second
    passes = voxels * (1 + 1 + 1 + 8 + 8 + 1)                                     # mask, K written and read, B written and read, out
    res = {"shape": list(SHAPE), "spacing_mm": list(SPACING), "mask_voxels_set": int(mask.sum()), "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "reach": {f"{r:g}mm": list(M.reach(SPACING, r)) for r in RADII}, **times, "min_max_over_repeats": spread,
           "copy_GBs": round(copy_rate / 1e9, 1), "contract_traffic_MB": round(2 * voxels / 1e6, 2),
           "contract_traffic_us": round(2 * voxels / copy_rate * 1e6, 2), "passes_traffic_MB": round(passes / 1e6, 1),
           "passes_traffic_us": round(passes / copy_rate * 1e6, 1), "scipy_edt_host_s": round(scipy_s, 2), "checked_against_restatement": checked}
    for r in RADII:
        res[f"ingest_margin_{r:g}mm_minus_ingest_us"] = round(times[f"ingest_margin_{r:g}mm_us"] - times["ingest_us"], 1)
        res[f"extract_shell_{r:g}mm_minus_extract_us"] = round(times[f"extract_shell_{r:g}mm_us"] - times["extract_us"], 1)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
