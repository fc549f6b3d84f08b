#!/usr/bin/env python
"""Time of the two pre-steps of the radiomics path (mmnn_sts_amd/radiomics.py: normalize_scan, resample_pair;
csrc/radiomics_resample.hip) on the workload of tools/radiomics_time.py: a 512 x 512 x 48 int16 scan (slope 0.25, inter -12.5) at
0.8 x 0.8 x 5 mm and the same ellipsoid ROI.

    python tools/radiomics_resample_time.py [--steps 10] [--warmup 3] [--repeats 3] [--json profiles/radiomics_resample_time.json]

Cases: `normalize` alone; `resample_1mm` (410 x 410 x 240) and `resample_2mm` (205 x 205 x 120).  Device times are HIP events after
warm-up with the calls queued back to back behind a spin kernel (device time alone), per case:
    step_us / step_rotating_us            the pre-step alone, with one buffer set and with 24 in turn
    kernels_us                            the per-kernel split of one call (torch.profiler, device time per kernel name)
    extract_us                            `mmnn_radiomics` (first order and GLCM, bin width 25) on the pre-step's output grid
against the traffic of the contract -- one read of the scan (and the mask), one write of the output(s) -- at the copy rate measured in
the same run (`copy_TBs`: a device-to-device copy of 256 MiB, bytes read plus bytes written over its time):
    contract_MB, contract_floor_us, step_over_floor
and `moved_MB`, what the kernels themselves read and write, their fp64 intermediates included.  `numpy_restatement_ms` is the host time
of tests/_radiomics_resample_ref.py on the same volume, whose output the device's is compared with bit for bit here too.
No target was set in advance: the capability is new."""
import argparse
import ctypes
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import _lib, radiomics  # noqa: E402
from mmnn_sts_amd.data import ingest  # noqa: E402
from tools.radiomics_time import BIN_WIDTH, MAX_BINS, ROTATING, SHAPE, copy_tbs, ellipsoid, kernel_split, queued_us  # noqa: E402

SPACING = (0.8, 0.8, 5.0)
SCALE = 100.0
COPY_BYTES = 256 << 20


def measure(named, a):
    for _, fn in named:
        for _ in range(a.warmup):
            fn()
    runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]         # the variants alternate inside a repeat
    times = {name: round(float(np.median([q[name] for q in runs])), 1) for name, _ in named}
    spread = {name: [round(min(q[name] for q in runs), 1), round(max(q[name] for q in runs), 1)] for name, _ in named}
    return times, spread


def rotate(fn):
    turn = [0]

    def step():
        turn[0] = (turn[0] + 1) % ROTATING
        fn(turn[0])
    return step


def extraction(vol, mask, a):
    """`mmnn_radiomics` on a float32 volume and a mask of one grid: (times, Ng, ROI voxels)."""
    r = radiomics.extract(vol, mask, vol.data.device, BIN_WIDTH, MAX_BINS)
    torch.cuda.synchronize()
    f = radiomics.unpack_block(r.block.cpu().numpy())
    assert not (f["empty"] or f["nonfinite"] or f["overflow"]), f
    desc = _lib.RadiomicsDesc(*vol.shape, vol.datatype, mask.datatype, vol.slope, vol.inter, mask.slope, mask.inter, BIN_WIDTH, MAX_BINS)
    stream = torch.cuda.current_stream().cuda_stream
    times, spread = measure((("extract_us", lambda: radiomics.enqueue(r, "first", desc, stream, vol.data.data_ptr(), mask.data.data_ptr())),), a)
    return {"extract_us": times["extract_us"], "extract_min_max": spread["extract_us"], "n_bins": f["n_bins"], "roi_voxels": f["n"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "radiomics_resample_time.json"))
    ap.add_argument("--no_host", action="store_true", help="skip the numpy restatement and the comparison with it")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from tests import _radiomics_resample_ref as P
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
    us_of = lambda nbytes: nbytes / (tbs * 1e12) * 1e6
    cases = {}

    # ---- normalise alone
    ws = torch.empty(L.mmnn_normalize_scan_workspace_bytes(*SHAPE), dtype=torch.uint8, device=dev)
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(ROTATING)]
    blocks = [torch.empty(_lib.NORMALIZE_RESULT_BYTES, dtype=torch.uint8, device=dev) for _ in range(ROTATING)]
    ndesc = _lib.NormalizeDesc(*SHAPE, s.datatype, s.slope, s.inter, SCALE, 0.0)

    def norm(k):
        _lib.check(L.mmnn_normalize_scan(ctypes.byref(ndesc), s.data.data_ptr(), outs[k].data_ptr(), blocks[k].data_ptr(), ws.data_ptr(), stream),
                   "mmnn_normalize_scan")

    for k in range(ROTATING):
        norm(k)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and all(torch.equal(blocks[0], b) for b in blocks[1:]), "two calls differ"
    times, spread = measure((("step_us", lambda: norm(0)), ("step_rotating_us", rotate(norm))), a)
    stats = radiomics.unpack_normalize(blocks[0].cpu().numpy())
    contract = scan.nbytes + n * 4
    case = {"out_shape": list(SHAPE), **times, "min_max_over_repeats": spread, "kernels_us": kernel_split(lambda: norm(0)),
            "contract_MB": round(contract / 1e6, 2), "contract_floor_us": round(us_of(contract), 1),
            "step_over_floor": round(times["step_us"] / us_of(contract), 1), "moved_MB": round((3 * scan.nbytes + n * 4) / 1e6, 1),
            "mean": stats["mean"], "sd": stats["sd"]}
    normalized = ingest.DeviceVolume(outs[0].view(torch.uint8), SHAPE, 16, 0.0, 0.0, aff)
    case.update(extraction(normalized, m, a))
    if not a.no_host:
        t = time.perf_counter()
        want = P.normalize(scan, (0.25, -12.5), SCALE)
        case["numpy_restatement_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        got = outs[0].cpu().numpy().reshape(SHAPE, order="F")
        assert np.array_equal(got, P.normalize(scan, (0.25, -12.5), SCALE, mean=stats["mean"], sd=stats["sd"])), "device and restatement differ"
        case["max_abs_difference_from_numpy_statistics"] = float(np.abs(got - want).max())
    cases["normalize"] = case
    del outs, blocks, normalized

    # ---- resample
    k_ = radiomics.resample_constants()
    for name, spacing in (("resample_1mm", 1.0), ("resample_2mm", 2.0)):
        g = radiomics.resample_grid(SHAPE, aff, spacing)
        host = radiomics.resample_tables(SHAPE, g)
        mx, my, mz = g.shape
        mo = mx * my * mz
        nbytes = radiomics.resample_workspace_bytes(SHAPE, g.shape)
        wss = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(ROTATING)]
        outs = [torch.empty(mo, dtype=torch.float32, device=dev) for _ in range(ROTATING)]
        oms = [torch.empty(mo, dtype=torch.uint8, device=dev) for _ in range(ROTATING)]
        tp = torch.from_numpy(host.view(np.uint8).copy()).to(dev)
        rdesc = _lib.ResampleDesc(*SHAPE, mx, my, mz, s.datatype, m.datatype, s.slope, s.inter, m.slope, m.inter, k_["pole"], k_["pole_gain"], k_["gain"],
                                  (ctypes.c_double * _lib.RESAMPLE_HORIZON)(*k_["pole_power"].tolist()))

        def res(k):
            _lib.check(L.mmnn_resample_pair(ctypes.byref(rdesc), s.data.data_ptr(), m.data.data_ptr(), host.ctypes.data, tp.data_ptr(), outs[k].data_ptr(),
                                            oms[k].data_ptr(), wss[k].data_ptr(), stream), "mmnn_resample_pair")

        for k in range(ROTATING):
            res(k)
        torch.cuda.synchronize()
        assert all(torch.equal(outs[0], o) for o in outs[1:]) and all(torch.equal(oms[0], o) for o in oms[1:]), "two calls differ"
        times, spread = measure((("step_us", lambda: res(0)), ("step_rotating_us", rotate(res))), a)
        contract = scan.nbytes + mask.nbytes + mo * 5
        t1, t2 = mx * SHAPE[1] * SHAPE[2], mx * my * SHAPE[2]
        # x prefilter: scan read, c+ written, read, c- written; y and z: 2 reads + 2 writes of coef each; the three gathers; the mask byte
        moved = scan.nbytes + 3 * n * 8 + 2 * 4 * n * 8 + (n + t1) * 8 + (t1 + t2) * 8 + t2 * 8 + mo * 4 + mo * 2
        case = {"out_shape": list(g.shape), **times, "min_max_over_repeats": spread, "kernels_us": kernel_split(lambda: res(0)),
                "contract_MB": round(contract / 1e6, 2), "contract_floor_us": round(us_of(contract), 1),
                "step_over_floor": round(times["step_us"] / us_of(contract), 1), "moved_MB": round(moved / 1e6, 1),
                "workspace_MB": round(nbytes / 1e6, 1), "outside_voxels": int(mo - np.prod([int(e["inside"].sum()) for e in P.split_tables(g.shape, host)]))}
        vol = ingest.DeviceVolume(outs[0].view(torch.uint8), g.shape, 16, 0.0, 0.0, g.affine)
        vm = ingest.DeviceVolume(oms[0], g.shape, 2, 1.0, 0.0, g.affine)
        case.update(extraction(vol, vm, a))
        if not a.no_host:
            t = time.perf_counter()
            want, wm = P.restate(scan, mask, g, host, k_, (0.25, -12.5))
            case["numpy_restatement_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            assert np.array_equal(outs[0].cpu().numpy().reshape(g.shape, order="F"), want), "device and restatement differ (scan)"
            assert np.array_equal(oms[0].cpu().numpy().reshape(g.shape, order="F"), wm), "device and restatement differ (mask)"
            case["equals_restatement"] = True
        cases[name] = case
        del wss, outs, oms, vol, vm
    res_ = {"shape": list(SHAPE), "spacing_mm": list(SPACING), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "buffer_sets": ROTATING,
            "copy_MB": COPY_BYTES >> 20, "copy_TBs": round(tbs, 2), "normalize_scale": SCALE, "bin_width": BIN_WIDTH,
            "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0), "cases": cases}
    print(json.dumps(res_), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res_, f, indent=1)


if __name__ == "__main__":
    main()
