#!/usr/bin/env python
"""Time of the RTSTRUCT mask path per volume (mmnn_sts_amd/data/rtstruct.py, ingest.rasterize_contours, csrc/rtstruct.hip) beside the
path it replaces for the same voxels, a DICOM mask series (decode + resample at the identity), in one run: a 512 x 512 x 48 int16 scan
whose tumour is a synth_nifti-style ellipsoid, traced on every slice it meets as one smooth polygon of 200-600 points (not the
run-rectangles of `synth_dicom.write_rtstruct`, which are a test device) and written as an RT Structure Set file.

    python tools/rtstruct_time.py [--steps 50] [--warmup 10] [--repeats 3] [--json profiles/rtstruct_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone), as in
tools/dicom_ingest_time.py:
    rasterize_us                 `mmnn_rasterize_contours` alone, contours on the device, the same 12.6 MB output every call (it stays in
                                 the 256 MB last-level cache: the warm figure)
    rasterize_rotating_us        ... with 24 output buffers in turn (302 MB: every call writes lines the cache no longer holds)
    rasterize_no_contours_us     leave-one-out: the same launch with n_contours = 0 -- the stores alone, no staging, no crossings
    rtstruct_mask_path_us        upload of the three arrays + rasterise + the three ingest passes (the scan already decoded)
    series_mask_path_us          the parent path for the same mask voxels as an 8-bit 0 / 255 series already on the device:
                                 decode + resample at the identity + the three ingest passes
    ingest_us                    the three ingest passes alone on the rasterised mask
    *_volume_us                  the two mask paths with the scan's own decode in front, i.e. a whole DICOM volume
The only bound that can be derived is the 12.6 MB the kernel must write, priced against the 6.29 TB/s measured HBM ceiling.  The host's
share is reported beside them: parsing the file, selecting the ROI and placing its contours on the scan's grid, against parsing the 48
slice headers of the mask series."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd.data import dicom, ingest, rtstruct, synth_dicom  # noqa: E402
from dicom_timing import best_ms, decode, ingest_passes, queued_us  # noqa: E402

HBM_TBS = 6.29
SHAPE = (512, 512, 48)
CENTRE, RADIUS = (262.3, 249.6, 23.4), (163.7, 151.2, 17.8)       # voxels: the ellipsoid meets 36 of the 48 slices
ROTATING = 24


def traced_ellipsoid(affine):
    """[(geometric type, (n, 3) LPS mm)]: per slice the ellipsoid's section as one polygon, 200-600 points by its circumference."""
    contours = []
    for k in range(SHAPE[2]):
        w = 1.0 - ((k - CENTRE[2]) / RADIUS[2]) ** 2
        if w <= 0.0:
            continue
        rx, ry = RADIUS[0] * np.sqrt(w), RADIUS[1] * np.sqrt(w)
        n = int(np.clip(round(np.pi * (rx + ry) / 1.7), 200, 600))
        t = 0.1 * k + 2.0 * np.pi * np.arange(n) / n
        idx = np.stack([CENTRE[0] + rx * np.cos(t), CENTRE[1] + ry * np.sin(t), np.full(n, float(k)), np.ones(n)], axis=1)
        contours.append(("CLOSED_PLANAR", (idx @ affine.T)[:, :3] * np.array([-1.0, -1.0, 1.0])))
    return contours


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="every figure is the median of this many windows of --steps calls")
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "rtstruct_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(1, 3000, SHAPE, dtype=np.int16)
    voxels = int(np.prod(SHAPE))
    affine = np.diag([0.7, 0.7, 3.0, 1.0])
    stream = torch.cuda.current_stream().cuda_stream
    with tempfile.TemporaryDirectory() as d:
        synth_dicom.write_series(os.path.join(d, "image"), scan, affine, 0.25, -12.5, seed=1)
        contours = traced_ellipsoid(affine)
        with open(os.path.join(d, "rs.dcm"), "wb") as f:
            f.write(synth_dicom.rtstruct_bytes([("Body", contours[:1]), ("GTV", contours)]))
        s_series = dicom.read_series(os.path.join(d, "image"))
        host = {"rtstruct_file_kB": round(os.path.getsize(os.path.join(d, "rs.dcm")) / 1e3, 1),
                "rtstruct_read_ms": best_ms(lambda: rtstruct.read(os.path.join(d, "rs.dcm"))),
                "rtstruct_read_header_only_ms": best_ms(lambda: rtstruct.read(os.path.join(d, "rs.dcm"), header_only=True))}
        cs = rtstruct.select(rtstruct.read(os.path.join(d, "rs.dcm")), "gtv")
        host["select_and_to_scan_index_ms"] = best_ms(lambda: rtstruct.to_scan_index(cs, s_series.shape, s_series.affine))
        arrays = rtstruct.to_scan_index(cs, s_series.shape, s_series.affine)[:3]
        per_slice = np.diff(arrays[2])
        counts = arrays[1][:, 1]

        # device: the scan's bytes as `decode_series` stages them; the contours as `stage_contours` uploads them
        pix_s = torch.from_numpy(np.concatenate(s_series.frames)).to("cuda")
        out_s = torch.empty(voxels * 2, dtype=torch.uint8, device="cuda")
        vol_s = ingest.DeviceVolume(out_s, SHAPE, 4, 0.25, -12.5, s_series.affine)      # (beside masks already on its grid)
        staged = ingest.stage_contours(arrays, vol_s, "cuda")
        masks = [torch.empty(voxels, dtype=torch.uint8, device="cuda") for _ in range(ROTATING)]
        plane = torch.empty((64, 64, 64), device="cuda")
        ext = torch.empty(3, dtype=torch.int32, device="cuda")
        ws = torch.empty(ingest.workspace_bytes(*SHAPE), dtype=torch.uint8, device="cuda")
        turn = [0]

        def rasterize():
            return ingest.rasterize_contours(staged, vol_s, out=masks[0])

        def rasterize_rotating():
            turn[0] = (turn[0] + 1) % ROTATING
            return ingest.rasterize_contours(staged, vol_s, out=masks[turn[0]])

        empty = ingest.stage_contours((np.zeros((0, 2)), np.zeros((0, 2), dtype=np.int32), np.zeros(SHAPE[2] + 1, dtype=np.int32)), vol_s, "cuda")

        def rasterize_no_contours():
            return ingest.rasterize_contours(empty, vol_s, out=masks[1])

        def rtstruct_mask_path():
            m = ingest.rasterize_contours(ingest.stage_contours(arrays, vol_s, "cuda"), vol_s, out=masks[0])
            ingest.ingest_volume(vol_s, m, plane, ext, ws, index_map=None)

        decode(s_series, pix_s, out_s, stream)
        rasterize()
        torch.cuda.synchronize()
        mask = masks[0].cpu().numpy().reshape(SHAPE, order="F")
        assert mask.any() and set(np.unique(mask)) == {0, 1}

        # the parent path: the same voxels as an 8-bit 0 / 255 mask series
        synth_dicom.write_series(os.path.join(d, "mask"), mask * np.uint8(255), affine, seed=2)
        host["mask_series_parse_ms"] = best_ms(lambda: dicom.read_series(os.path.join(d, "mask")))
        m_series = dicom.read_series(os.path.join(d, "mask"))
        pix_m = torch.from_numpy(np.concatenate(m_series.frames)).to("cuda")
        out_m = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        resampled = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        vol_m = ingest.DeviceVolume(out_m, SHAPE, 2, 1.0, 0.0, m_series.affine, from_dicom=True)
        drawn = ingest.DeviceVolume(masks[0], SHAPE, 2, 1.0, 0.0, s_series.affine)

        def series_mask_path():
            decode(m_series, pix_m, out_m, stream)
            m = ingest.resample_mask(vol_m, SHAPE, ingest.IDENTITY_MAP, ingest.DICOM_MASK_THRESHOLD, out=resampled)
            ingest.ingest_volume(vol_s, m, plane, ext, ws, index_map=None)

        def bare_ingest():
            ingest_passes(vol_s, drawn, plane, ext, ws, stream)

        def rtstruct_volume():
            decode(s_series, pix_s, out_s, stream)
            rtstruct_mask_path()

        def series_volume():
            decode(s_series, pix_s, out_s, stream)
            series_mask_path()

        for _ in range(a.warmup):
            rtstruct_mask_path()
        torch.cuda.synchronize()
        kept_r, plane_r = ext.cpu().tolist(), plane.clone()
        for _ in range(a.warmup):
            series_mask_path()
        torch.cuda.synchronize()
        assert kept_r == ext.cpu().tolist() and min(kept_r) > 0 and torch.equal(plane_r, plane), (kept_r, ext)
        for fn in (rasterize, rasterize_rotating, rasterize_no_contours, bare_ingest, rtstruct_volume, series_volume):
            for _ in range(a.warmup):
                fn()
        named = (("rasterize_us", rasterize), ("rasterize_rotating_us", rasterize_rotating), ("rasterize_no_contours_us", rasterize_no_contours),
                 ("rtstruct_mask_path_us", rtstruct_mask_path), ("series_mask_path_us", series_mask_path), ("ingest_us", bare_ingest),
                 ("rtstruct_volume_us", rtstruct_volume), ("series_volume_us", series_volume))
        runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]      # the figures in turn, `repeats` times over
        times = {name: round(float(np.median([r[name] for r in runs])), 1) for name, _ in named}
        spread = {name: [round(min(r[name] for r in runs), 1), round(max(r[name] for r in runs), 1)] for name, _ in named}
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "slices_with_a_contour": int((per_slice > 0).sum()),
           "points_per_contour": [int(counts.min()), int(counts.max())], "points": int(counts.sum()), "voxels_set": int(mask.sum()),
           "repeats": a.repeats, **times, "min_max_over_repeats": spread, "write_MB": round(voxels / 1e6, 2), "write_hbm_floor_us": round(voxels / (HBM_TBS * 1e12) * 1e6, 2),
           "rasterize_rotating_share_of_hbm_ceiling": round(voxels / (times["rasterize_rotating_us"] * 1e-6) / 1e12 / HBM_TBS, 3),
           "rtstruct_minus_series_mask_path_us": round(times["rtstruct_mask_path_us"] - times["series_mask_path_us"], 1),
           "host_per_volume": host}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
