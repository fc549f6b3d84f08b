#!/usr/bin/env python
"""Time of the mesh-based shape call (mmnn_sts_amd/radiomics.py, csrc/radiomics_mesh.hip) on the workload of tools/radiomics_time.py:
a 512 x 512 x 48 int16 scan (slope 0.25, inter -12.5), the same ellipsoid ROI, bin_width 25, max_bins 256, under an anisotropic linear part.

    python tools/radiomics_mesh_time.py [--steps 10] [--warmup 3] [--repeats 3] [--json profiles/radiomics_mesh_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone):
    extract_three_us       `mmnn_radiomics` + `mmnn_radiomics_texture` + `mmnn_radiomics_zones`, one buffer set: the figure of
                           profiles/radiomics_zones_time.json measured again in this run
    extract_four_us        the three calls + `mmnn_radiomics_mesh`;  mesh_us is the difference
    kernels_us             the per-kernel split of one quadruple of calls (torch.profiler, device time per kernel name, averaged over the calls)
    vertices, pairs        V as the device counted it and V (V + 1) / 2, the unordered pairs with the self-pairs
    pairs_per_s            pairs over the pair kernel's device time.  The kernel computes whole 256 x 256 tiles, the diagonal ones in both
                           orders, so it evaluates tile_pairs = 65536 T (T + 1) / 2 scores; evaluated_per_s counts those
    fp64_valu_fraction     evaluated_per_s x 8 fp64 operations per score (3 subtractions, 3 products, 2 additions; no contraction) over the
                           fp64 vector rate of the chip, 256 CUs x 4 SIMDs x 16 lanes per clock at the clock given by --mhz
No target was set in advance: the capability is new."""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import radiomics  # noqa: E402
from mmnn_sts_amd.data import ingest  # noqa: E402
from tools.radiomics_time import BIN_WIDTH, MAX_BINS, SHAPE, ellipsoid, enqueuer, kernel_split, queued_us  # noqa: E402

LINEAR = np.diag([0.78, 0.78, 5.0])
FP64_OPS_PER_SCORE = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mhz", type=float, default=2400.0, help="the clock the fp64 vector rate is taken at")
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "radiomics_mesh_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(100, 3000, SHAPE, dtype=np.int16)
    mask = ellipsoid()
    dev = torch.device("cuda", 0)
    aff = np.eye(4)
    aff[:3, :3] = LINEAR
    s = dataclasses.replace(ingest.upload(scan, dev, 0.25, -12.5), affine=aff)
    m = dataclasses.replace(ingest.upload(mask, dev), affine=aff)
    r = radiomics.extract(s, m, dev, BIN_WIDTH, MAX_BINS, classes=radiomics.TEXTURE_CLASSES, glszm=True, mesh=True)
    again = radiomics.extract(s, m, dev, BIN_WIDTH, MAX_BINS, mesh=True)
    torch.cuda.synchronize()
    fields = radiomics.unpack_block(r.block.cpu().numpy())
    assert not (fields["empty"] or fields["nonfinite"] or fields["overflow"]), fields
    assert torch.equal(r.mesh, again.mesh) and torch.equal(r.mesh_cfg, again.mesh_cfg), "two calls differ"
    del again
    mesh = radiomics.unpack_mesh(r.mesh.cpu().numpy())
    feats = radiomics.finish(r)
    assert np.array_equal(r.linear, LINEAR)                # what the mesh call is enqueued under
    call = enqueuer(s, m)

    def three():
        call(r, "first", "texture", "zones")

    def four():
        call(r, "first", "texture", "zones", "mesh")

    named = (("extract_three_us", three), ("extract_four_us", four))
    for _, fn in named:
        for _ in range(a.warmup):
            fn()
    runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]          # the variants alternate inside a repeat
    times = {name: round(float(np.median([q[name] for q in runs])), 1) for name, _ in named}
    spread = {name: [round(min(q[name] for q in runs), 1), round(max(q[name] for q in runs), 1)] for name, _ in named}
    kernels = kernel_split(four)
    mesh_kernels = {k: v for k, v in kernels.items() if "mesh_" in k}
    V = mesh["n_vertices"]
    T = (V + 255) // 256
    pairs, evaluated = V * (V + 1) // 2, 65536 * T * (T + 1) // 2
    pair_us = next((v for k, v in mesh_kernels.items() if "mesh_pair_kernel" in k), None)
    rate = 256 * 4 * 16 * a.mhz * 1e6
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "roi_voxels": fields["n"], "linear": LINEAR.tolist(),
           "vertices": V, "triangles": mesh["n_triangles"], "volume48": mesh["volume48"], "pairs": pairs, "tile_pairs_evaluated": evaluated,
           **times, "mesh_us": round(times["extract_four_us"] - times["extract_three_us"], 1), "min_max_over_repeats": spread,
           "kernels_us": kernels, "mesh_kernels_us": mesh_kernels,
           "pairs_per_s": None if not pair_us else round(pairs / (pair_us * 1e-6), 1),
           "evaluated_per_s": None if not pair_us else round(evaluated / (pair_us * 1e-6), 1),
           "fp64_valu_lane_ops_per_s": rate, "fp64_ops_per_score": FP64_OPS_PER_SCORE, "mhz_assumed": a.mhz,
           "fp64_valu_fraction": None if not pair_us else round(evaluated / (pair_us * 1e-6) * FP64_OPS_PER_SCORE / rate, 3),
           "mesh_workspace_MB": round(r.mesh_workspace.numel() / 1e6, 1),
           "features": {k: v for k, v in feats.items() if k.startswith("original_shape_")}}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
