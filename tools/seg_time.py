#!/usr/bin/env python
"""Time of the DICOM SEG mask path per volume (mmnn_sts_amd/data/seg.py, ingest.unpack_frames, csrc/seg.hip) beside the path it
replaces for the same voxels, a DICOM mask series (decode + resample at the identity), in one run: a 512 x 512 x 48 int16 scan whose
tumour is an ellipsoid that meets 20 of the 48 slices, written as a BINARY Segmentation object with a decoy segment
(`synth_dicom.write_seg`: 20 + 1 frames, shuffled, bit-packed back to back).

    python tools/seg_time.py [--steps 50] [--warmup 10] [--repeats 3] [--json profiles/seg_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone), as in
tools/rtstruct_time.py; the figures are taken in turn, `repeats` times over, so the two paths alternate within one run:
    unpack_us                    `mmnn_unpack_frames` alone, frames on the device, the same 12.6 MB output every call (it stays in the
                                 256 MB last-level cache: the warm figure)
    unpack_rotating_us           ... with 24 output buffers in turn (302 MB: every call writes lines the cache no longer holds)
    unpack_no_frames_us          leave-one-out: the same launch with n_refs = 0 -- the stores alone
    series_mask_us               the parent path to the same mask bytes, the 8-bit 0 / 255 series already on the device: decode +
                                 resample at the identity
    seg_mask_path_us             upload of refs, slice_first and the bit stream + unpack + the three ingest passes (scan already decoded)
    series_mask_path_us          decode + resample at the identity + the three ingest passes, the mask series already on the device
    ingest_us                    the three ingest passes alone on the unpacked mask
The bytes the contract moves (the mask written once, the listed frames' bits and the two index arrays read once) are priced against
the 6.29 TB/s measured HBM ceiling.  The host's share is reported beside them: parsing the file, selecting the segment and placing its
frames against the scan, against parsing the 48 slice headers of the mask series."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd.data import dicom, ingest, seg, synth_dicom  # noqa: E402
from dicom_timing import best_ms, decode, ingest_passes, queued_us  # noqa: E402

HBM_TBS = 6.29
SHAPE = (512, 512, 48)
CENTRE, RADIUS = (262.3, 249.6, 23.4), (163.7, 151.2, 10.2)       # voxels: the ellipsoid meets slices 14 .. 33, 20 of the 48
ROTATING = 24


def ellipsoid():
    g = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in SHAPE], indexing="ij", sparse=True)
    return (sum(((v - c) / r) ** 2 for v, c, r in zip(g, CENTRE, RADIUS)) <= 1.0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="every figure is the median of this many windows of --steps calls")
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "seg_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(1, 3000, SHAPE, dtype=np.int16)
    voxels = int(np.prod(SHAPE))
    affine = np.diag([0.7, 0.7, 3.0, 1.0])
    stream = torch.cuda.current_stream().cuda_stream
    mask = ellipsoid()
    occupied = int(mask.any(axis=(0, 1)).sum())
    assert occupied == 20, occupied
    with tempfile.TemporaryDirectory() as d:
        synth_dicom.write_series(os.path.join(d, "image"), scan, affine, 0.25, -12.5, seed=1)
        path = synth_dicom.write_seg(os.path.join(d, "seg.dcm"), mask, affine, "GTV", ("Body",), seed=3)
        s_series = dicom.read_series(os.path.join(d, "image"))
        host = {"seg_file_kB": round(os.path.getsize(path) / 1e3, 1), "seg_read_ms": best_ms(lambda: seg.read(path)),
                "seg_read_header_only_ms": best_ms(lambda: seg.read(path, header_only=True))}
        fs = seg.select(seg.read(path), "gtv")
        host["select_and_to_scan_ms"] = best_ms(lambda: seg.to_scan(seg.select(fs, None), s_series.shape, s_series.affine))
        place = seg.to_scan(fs, s_series.shape, s_series.affine)
        assert place.on_scan and len(place.refs) == occupied

        # device: the scan's bytes as `decode_series` stages them; the frames as `stage_frames` uploads them
        pix_s = torch.from_numpy(np.concatenate(s_series.frames)).to("cuda")
        out_s = torch.empty(voxels * 2, dtype=torch.uint8, device="cuda")
        vol_s = ingest.DeviceVolume(out_s, SHAPE, 4, 0.25, -12.5, s_series.affine, from_dicom=True)
        staged = ingest.stage_frames(fs, vol_s, "cuda")
        masks = [torch.empty(voxels, dtype=torch.uint8, device="cuda") for _ in range(ROTATING)]
        plane = torch.empty((64, 64, 64), device="cuda")
        ext = torch.empty(3, dtype=torch.int32, device="cuda")
        ws = torch.empty(ingest.workspace_bytes(*SHAPE), dtype=torch.uint8, device="cuda")
        turn = [0]

        def unpack():
            return ingest.unpack_frames(staged, vol_s, out=masks[0])

        def unpack_rotating():
            turn[0] = (turn[0] + 1) % ROTATING
            return ingest.unpack_frames(staged, vol_s, out=masks[turn[0]])

        empty = ingest.stage_frames((np.zeros(0, dtype=np.uint8), 0, np.zeros(0, dtype=np.int32), np.zeros(SHAPE[2] + 1, dtype=np.int32)), vol_s, "cuda")

        def unpack_no_frames():
            return ingest.unpack_frames(empty, vol_s, out=masks[1])

        def _ingest(s, m):
            ingest_passes(s, m, plane, ext, ws, stream)

        def seg_mask_path():
            m = ingest.unpack_frames(ingest.stage_frames(fs, vol_s, "cuda"), vol_s, out=masks[0])
            _ingest(vol_s, m)

        decode(s_series, pix_s, out_s, stream)
        unpack()
        torch.cuda.synchronize()
        got = masks[0].cpu().numpy().reshape(SHAPE, order="F")
        assert np.array_equal(got, mask), "the unpacked mask is not the one written"

        # the parent path: the same voxels as an 8-bit 0 / 255 mask series
        synth_dicom.write_series(os.path.join(d, "mask"), mask * np.uint8(255), affine, seed=2)
        host["mask_series_parse_ms"] = best_ms(lambda: dicom.read_series(os.path.join(d, "mask")))
        m_series = dicom.read_series(os.path.join(d, "mask"))
        pix_m = torch.from_numpy(np.concatenate(m_series.frames)).to("cuda")
        out_m = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        resampled = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        vol_m = ingest.DeviceVolume(out_m, SHAPE, 2, 1.0, 0.0, m_series.affine, from_dicom=True)
        unpacked = ingest.DeviceVolume(masks[0], SHAPE, 2, 1.0, 0.0, s_series.affine)

        def series_mask():
            decode(m_series, pix_m, out_m, stream)
            return ingest.resample_mask(vol_m, SHAPE, ingest.IDENTITY_MAP, ingest.DICOM_MASK_THRESHOLD, out=resampled)

        def series_mask_path():
            _ingest(vol_s, series_mask())

        def bare_ingest():
            _ingest(vol_s, unpacked)

        for _ in range(a.warmup):
            seg_mask_path()
        torch.cuda.synchronize()
        kept_s, plane_s = ext.cpu().tolist(), plane.clone()
        for _ in range(a.warmup):
            series_mask_path()
        torch.cuda.synchronize()
        assert kept_s == ext.cpu().tolist() and min(kept_s) > 0 and torch.equal(plane_s, plane), (kept_s, ext)
        assert torch.equal(resampled, masks[0])
        named = (("unpack_us", unpack), ("unpack_rotating_us", unpack_rotating), ("unpack_no_frames_us", unpack_no_frames), ("series_mask_us", series_mask),
                 ("seg_mask_path_us", seg_mask_path), ("series_mask_path_us", series_mask_path), ("ingest_us", bare_ingest))
        for _, fn in named:
            for _ in range(a.warmup):
                fn()
        runs = [{name: queued_us(fn, a.steps) for name, fn in named} for _ in range(a.repeats)]      # the figures in turn, `repeats` times over
        times = {name: round(float(np.median([r[name] for r in runs])), 1) for name, _ in named}
        spread = {name: [round(min(r[name] for r in runs), 1), round(max(r[name] for r in runs), 1)] for name, _ in named}
    read_bytes = occupied * SHAPE[0] * SHAPE[1] // 8 + 4 * (occupied + SHAPE[2] + 1)
    moved = voxels + read_bytes
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "occupied_slices": occupied, "frames_in_file": int(fs.n_frames),
           "voxels_set": int(mask.sum()), **times, "min_max_over_repeats": spread, "write_MB": round(voxels / 1e6, 2),
           "read_MB": round(read_bytes / 1e6, 3), "contract_hbm_floor_us": round(moved / (HBM_TBS * 1e12) * 1e6, 2),
           "unpack_share_of_hbm_ceiling": round(moved / (times["unpack_us"] * 1e-6) / 1e12 / HBM_TBS, 3),
           "unpack_rotating_share_of_hbm_ceiling": round(moved / (times["unpack_rotating_us"] * 1e-6) / 1e12 / HBM_TBS, 3),
           "unpack_minus_series_mask_us": round(times["unpack_us"] - times["series_mask_us"], 1),
           "seg_minus_series_mask_path_us": round(times["seg_mask_path_us"] - times["series_mask_path_us"], 1),
           "host_per_volume": host}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
