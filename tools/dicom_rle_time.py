#!/usr/bin/env python
"""Time of the RLE Lossless path per volume (mmnn_sts_amd/data/dicom.py, ingest.decode_series, csrc/dicom_rle.hip) beside the uncompressed
DICOM path on the same voxels, in one run: the 512 x 512 x 48 int16 series with an 8-bit 0 / 255 box mask series of
tools/dicom_ingest_time.py, written once uncompressed and once with `transfer_syntax="rle"`, and the ellipsoid ROI of
tools/radiomics_time.py as an 8-bit RLE series on its own.

    python tools/dicom_rle_time.py [--steps 50] [--warmup 10] [--json profiles/dicom_rle_time.json]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (tools/dicom_timing.py):
    expand_us            `mmnn_rle_expand` alone, payload and segment table already on the device, the same buffers every call
    expand_rotating_us   the same over 24 buffer sets in turn (payload, table, words, workspace, status), so that no call finds its
                         predecessor's lines in the last-level cache
    expand_floor_us      reading the compressed bytes and writing the words, once each, at the copy rate measured in this run
    decode_us            `mmnn_decode_slices` alone on the same voxels (what follows the expansion unchanged)
    native_device_us     the uncompressed path: decode of scan and mask, the mask's resample at the identity, the three ingest passes
                         (tools/dicom_ingest_time.py's dicom_device_us)
    rle_device_us        the same with `mmnn_rle_expand` in front of each decode
The host's share: parsing the series (headers, and for RLE the 64-byte fragment headers), `decode_series` as a whole (stage, upload,
enqueue, and for RLE the status read-back, which waits for the device), and the read-back alone on an idle device."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnn_sts_amd import _lib  # noqa: E402
from mmnn_sts_amd.data import dicom, ingest, synth_dicom  # noqa: E402
from dicom_timing import best_ms, decode, queued_us  # noqa: E402
from radiomics_time import ROTATING, copy_tbs, ellipsoid, kernel_split  # noqa: E402

SHAPE = (512, 512, 48)
BOX = ((96, 101, 4), (416, 411, 43))


class Staged:
    """An RLE series on the device as `decode_series` stages it, with the buffers `mmnn_rle_expand` writes."""

    def __init__(self, series):
        x, y, z = series.shape
        planes = series.bits_allocated // 8
        starts = np.zeros(z + 1, dtype=np.int64)
        np.cumsum([(f.size + 15) // 16 * 16 for f in series.frames], out=starts[1:])
        payload = np.zeros(int(starts[-1]), dtype=np.uint8)
        table = np.stack([np.asarray(t, dtype=np.int64) for t in series.segments])
        for k, f in enumerate(series.frames):
            payload[starts[k]:starts[k] + f.size] = f
            table[k, :, 0] += starts[k]
        self.series, self.payload_bytes = series, int(payload.size)
        self.payload, self.table = torch.from_numpy(payload).to("cuda"), torch.from_numpy(table).to("cuda")
        self.words = torch.empty(x * y * z * planes, dtype=torch.uint8, device="cuda")
        self.status = torch.empty(z, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(_lib.count("mmnn_rle_workspace_bytes", x, y, z, series.bits_allocated), dtype=torch.uint8, device="cuda")
        self.desc = _lib.RleDesc(x, y, z, series.bits_allocated, self.payload_bytes)

    def expand(self, stream):
        _lib.check(_lib.lib().mmnn_rle_expand(ctypes.byref(self.desc), self.payload.data_ptr(), self.table.data_ptr(), self.words.data_ptr(),
                                              self.status.data_ptr(), self.ws.data_ptr(), stream), "mmnn_rle_expand")


def expand_times(series, native, steps, warmup, stream, tbs):
    """The figures of `mmnn_rle_expand` on one series; `native`: its uncompressed twin, whose bytes the words must equal."""
    sets = [Staged(series) for _ in range(ROTATING)]
    one = sets[0]
    for _ in range(warmup):
        one.expand(stream)
    torch.cuda.synchronize()
    assert not one.status.cpu().any() and one.words.cpu().numpy().tobytes() == b"".join(f.tobytes() for f in native.frames)
    turn = [0]

    def rotating():
        sets[turn[0] % ROTATING].expand(stream)
        turn[0] += 1

    for _ in range(ROTATING):
        rotating()
    words_bytes, native_bytes = one.words.numel(), sum(f.size for f in native.frames)
    readback = []
    for _ in range(20):
        torch.cuda.synchronize()
        t = time.perf_counter()
        one.status.cpu()
        readback.append((time.perf_counter() - t) * 1e6)
    res = {"expand_us": round(queued_us(lambda: one.expand(stream), steps), 1), "expand_rotating_us": round(queued_us(rotating, steps), 1),
           "expand_floor_us": round((one.payload_bytes + words_bytes) / (tbs * 1e12) * 1e6, 2),
           "uploaded_bytes_rle": one.payload_bytes + one.table.numel() * 8, "uploaded_bytes_native": native_bytes,
           "compression_ratio": round(native_bytes / sum(f.size for f in series.frames), 3),
           "status_readback_idle_us": round(min(readback), 1), "kernels_us": kernel_split(lambda: one.expand(stream))}
    return res, one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "dicom_rle_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    scan = rng.integers(1, 3000, SHAPE, dtype=np.int16)
    mask = np.zeros(SHAPE, dtype=np.uint8)
    (x0, y0, z0), (x1, y1, z1) = BOX
    mask[x0:x1, y0:y1, z0:z1] = 1
    voxels = int(np.prod(SHAPE))
    stream = torch.cuda.current_stream().cuda_stream
    tbs = copy_tbs(a.steps)
    with tempfile.TemporaryDirectory() as d:
        affine = np.diag([0.7, 0.7, 3.0, 1.0])
        path = lambda *p: os.path.join(d, *p)
        for syntax in ("native", "rle"):
            synth_dicom.write_series(path(syntax, "image"), scan, affine, 0.25, -12.5, seed=1, transfer_syntax=syntax)
            synth_dicom.write_series(path(syntax, "mask"), mask * np.uint8(255), affine, seed=2, transfer_syntax=syntax)
            synth_dicom.write_series(path(syntax, "roi"), ellipsoid() * np.uint8(255), affine, seed=3, transfer_syntax=syntax)
        read = lambda syntax, what, **kw: dicom.read_series(path(syntax, what), **kw)
        host = {f"parse_{s}_ms": best_ms(lambda: (read(s, "image"), read(s, "mask")), sync=True) for s in ("native", "rle")}
        series = {(s, w): read(s, w) for s in ("native", "rle") for w in ("image", "mask", "roi")}
        for s in ("native", "rle"):
            host[f"stage_upload_decode_{s}_ms"] = best_ms(lambda: (ingest.upload(series[s, "image"], "cuda"), ingest.upload(series[s, "mask"], "cuda")), sync=True)

        scan_res, rle_s = expand_times(series["rle", "image"], series["native", "image"], a.steps, a.warmup, stream, tbs)
        roi_res, _ = expand_times(series["rle", "roi"], series["native", "roi"], a.steps, a.warmup, stream, tbs)
        mask_res, rle_m = expand_times(series["rle", "mask"], series["native", "mask"], a.steps, a.warmup, stream, tbs)

        # the uncompressed path exactly as tools/dicom_ingest_time.py queues it, and the RLE path with the expansion in front
        s_series, m_series = series["native", "image"], series["native", "mask"]
        pix_s = torch.from_numpy(np.concatenate(s_series.frames)).to("cuda")
        pix_m = torch.from_numpy(np.concatenate(m_series.frames)).to("cuda")
        out_s = torch.empty(voxels * 2, dtype=torch.uint8, device="cuda")
        out_m = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        resampled = torch.empty(voxels, dtype=torch.uint8, device="cuda")
        plane = torch.empty((64, 64, 64), device="cuda")
        ext = torch.empty(3, dtype=torch.int32, device="cuda")
        ws = torch.empty(ingest.workspace_bytes(*SHAPE), dtype=torch.uint8, device="cuda")
        vol_s = ingest.DeviceVolume(out_s, SHAPE, 4, 0.25, -12.5)
        vol_m = ingest.DeviceVolume(out_m, SHAPE, 2, 1.0, 0.0, m_series.affine, from_dicom=True)

        def behind(words_s, words_m):
            decode(s_series, words_s, out_s, stream)
            decode(m_series, words_m, out_m, stream)
            m = ingest.resample_mask(vol_m, SHAPE, ingest.IDENTITY_MAP, ingest.DICOM_MASK_THRESHOLD, out=resampled)
            ingest.ingest_volume(vol_s, m, plane, ext, ws)

        def native_volume():
            behind(pix_s, pix_m)

        def rle_volume():
            rle_s.expand(stream)
            rle_m.expand(stream)
            behind(rle_s.words, rle_m.words)

        for _ in range(a.warmup):
            native_volume()
        torch.cuda.synchronize()
        kept, plane_n = ext.cpu().tolist(), plane.clone()
        for _ in range(a.warmup):
            rle_volume()
        torch.cuda.synchronize()
        assert kept == ext.cpu().tolist() == [b - a_ for a_, b in zip(*BOX)] and torch.equal(plane_n, plane), (kept, ext)
        decode_us = [queued_us(lambda: decode(s_series, pix_s, out_s, stream), a.steps) for _ in range(3)]
        native_us = [queued_us(native_volume, a.steps) for _ in range(3)]
        rle_us = [queued_us(rle_volume, a.steps) for _ in range(3)]
    res = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "copy_TBs": round(tbs, 2), "rotating_sets": ROTATING,
           "scan_int16": scan_res, "box_mask_uint8": mask_res, "ellipsoid_mask_uint8": roi_res,
           "decode_us": [round(v, 1) for v in decode_us], "native_device_us": [round(v, 1) for v in native_us],
           "rle_device_us": [round(v, 1) for v in rle_us], "rle_minus_native_us": round(min(rle_us) - min(native_us), 1),
           "host_per_volume": host}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
