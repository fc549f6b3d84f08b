#!/usr/bin/env python
"""Time of the DICOM path per volume (mmnn_sts_amd/data/dicom.py, ingest.decode_series, csrc/dicom.hip) beside the NIfTI ingest of the
same voxels, in one run: a 512 x 512 x 48 int16 series with an 8-bit 0 / 255 mask series, written by synth_dicom, against the int16
NIfTI scan with a 0 / 1 mask.

    python tools/dicom_ingest_time.py [--steps 50] [--warmup 10] [--json profiles/dicom_ingest_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (device time alone), as in
tools/ingest_time.py:
    decode_us            `mmnn_decode_slices` alone on the scan's bytes already on the device (one read and one write of the volume),
                         the same two 25 MB buffers every call: they fit the 256 MB last-level cache, so this is the warm figure
    dicom_device_us      decode of scan and mask, the mask's resample at the identity, the three ingest passes
    nifti_device_us      the three ingest passes on the same voxels (the NIfTI path has nothing in front of them)
Bytes are the algorithmic HBM traffic computed from the shapes, priced against the 6.29 TB/s measured HBM ceiling of the MI355X.  The
host's share per volume is reported beside them: parsing the 2 x 48 slice headers and mapping the files, and `decode_series` (the copy
of the slices into one pinned buffer, the upload and the enqueue) against gunzip + parse + upload of the two .nii.gz files."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd.data import dicom, ingest, nifti, synth_dicom  # noqa: E402
from dicom_timing import best_ms, decode, queued_us  # noqa: E402

HBM_TBS = 6.29
SHAPE = (512, 512, 48)
BOX = ((96, 101, 4), (416, 411, 43))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "dicom_ingest_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(1, 3000, SHAPE, dtype=np.int16)
    mask = np.zeros(SHAPE, dtype=np.uint8)
    (x0, y0, z0), (x1, y1, z1) = BOX
    mask[x0:x1, y0:y1, z0:z1] = 1
    voxels = int(np.prod(SHAPE))
    with tempfile.TemporaryDirectory() as d:
        affine = np.diag([0.7, 0.7, 3.0, 1.0])
        synth_dicom.write_series(os.path.join(d, "image"), scan, affine, 0.25, -12.5, seed=1)
        synth_dicom.write_series(os.path.join(d, "mask"), mask * np.uint8(255), affine, seed=2)
        ps = nifti.write(os.path.join(d, "scan.nii.gz"), scan, 0.25, -12.5, affine=affine)
        pm = nifti.write(os.path.join(d, "mask.nii.gz"), mask, affine=affine)
        host = {"dicom_parse_ms": best_ms(lambda: (dicom.read_series(os.path.join(d, "image")), dicom.read_series(os.path.join(d, "mask"))), sync=True),
                "nifti_gunzip_parse_ms": best_ms(lambda: (nifti.read(ps), nifti.read(pm)), sync=True)}
        s_series, m_series = dicom.read_series(os.path.join(d, "image")), dicom.read_series(os.path.join(d, "mask"))
        s_nifti, m_nifti = nifti.read(ps), nifti.read(pm)
        host["dicom_stage_upload_decode_ms"] = best_ms(lambda: (ingest.upload(s_series, "cuda"), ingest.upload(m_series, "cuda")), sync=True)
        host["nifti_upload_ms"] = best_ms(lambda: (ingest.upload(s_nifti, "cuda"), ingest.upload(m_nifti, "cuda")), sync=True)

        # device: the slices' bytes as `decode_series` stages them, then the calls it makes
        def staged(series):
            return torch.from_numpy(np.concatenate(series.frames)).to("cuda")

        pix_s, pix_m = staged(s_series), staged(m_series)
        out_s = torch.empty(voxels * 2, dtype=torch.uint8, device="cuda")
        out_m = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        resampled = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        plane = torch.empty((64, 64, 64), device="cuda")
        ext = torch.empty(3, dtype=torch.int32, device="cuda")
        ws = torch.empty(ingest.workspace_bytes(*SHAPE), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        vol_s = ingest.DeviceVolume(out_s, SHAPE, 4, 0.25, -12.5)      # (the decoded scan beside a mask already on its grid)
        vol_m = ingest.DeviceVolume(out_m, SHAPE, 2, 1.0, 0.0, m_series.affine, from_dicom=True)
        nif_s, nif_m = ingest.upload(s_nifti, "cuda"), ingest.upload(m_nifti, "cuda")

        def dicom_volume():
            decode(s_series, pix_s, out_s, stream)
            decode(m_series, pix_m, out_m, stream)
            m = ingest.resample_mask(vol_m, SHAPE, ingest.IDENTITY_MAP, ingest.DICOM_MASK_THRESHOLD, out=resampled)
            ingest.ingest_volume(vol_s, m, plane, ext, ws)

        def nifti_volume():
            ingest.ingest_volume(nif_s, nif_m, plane, ext, ws)

        for _ in range(a.warmup):
            dicom_volume()
        torch.cuda.synchronize()
        kept_d, plane_d = ext.cpu().tolist(), plane.clone()
        for _ in range(a.warmup):
            nifti_volume()
        torch.cuda.synchronize()
        assert kept_d == ext.cpu().tolist() == [b - a_ for a_, b in zip(*BOX)] and torch.equal(plane_d, plane), (kept_d, ext)
        decode_us = queued_us(lambda: decode(s_series, pix_s, out_s, stream), a.steps)
        dicom_us = queued_us(dicom_volume, a.steps)
        nifti_us = queued_us(nifti_volume, a.steps)
    decode_bytes = voxels * 4                                   # int16 read once, written once
    extra_bytes = decode_bytes + voxels * 2 + voxels * 2        # + the mask's decode (1 + 1) and its identity resample (1 + 1)
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup,
           "decode_us": round(decode_us, 1), "decode_MB": round(decode_bytes / 1e6, 2),
           "decode_hbm_floor_us": round(decode_bytes / (HBM_TBS * 1e12) * 1e6, 2),
           "decode_share_of_hbm_ceiling": round(decode_bytes / (decode_us * 1e-6) / 1e12 / HBM_TBS, 3),
           "dicom_device_us": round(dicom_us, 1), "nifti_device_us": round(nifti_us, 1), "dicom_minus_nifti_us": round(dicom_us - nifti_us, 1),
           "extra_MB_in_front_of_the_ingest": round(extra_bytes / 1e6, 2), "host_per_volume": host}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
