#!/usr/bin/env python
"""Time of the JPEG Lossless path per volume (mmnn_sts_amd/data/dicom.py, ingest.decode_series, csrc/dicom_jpegll.hip) beside the
uncompressed and the RLE Lossless DICOM paths on the same voxels, in one run: a 512 x 512 x 48 int16 series of full-range noise (the
worst case: about 17 bits a sample, a stuffed zero every 128 bytes), a smooth int16 series (the ellipsoid of tools/radiomics_time.py at
1000 over 0, plus noise of 0..15), and the two 8-bit 0 / 255 masks of tools/dicom_rle_time.py.

    python tools/dicom_jpegll_time.py [--steps 20] [--warmup 3] [--json profiles/dicom_jpegll_time.json] [--parent_us 143.1]

Device times are HIP events after warm-up with the calls queued back to back behind a spin kernel (tools/dicom_timing.py):
    decode_us            `mmnn_jpegll_decode` alone, payload and frame records already on the device, the same buffers every call
    decode_rotating_us   the same over 24 buffer sets in turn, so that no call finds its predecessor's lines in the last-level cache
    decode_floor_us      reading the compressed bytes and writing the words, once each, at the copy rate measured in this run
    native_device_us     the uncompressed path: `mmnn_decode_slices` of scan and mask, the mask's resample at the identity, the three
                         ingest passes (tools/dicom_ingest_time.py's dicom_device_us); three runs, so that their spread shows
    rle_device_us        the same with `mmnn_rle_expand` in front of each decode
    jpegll_device_us     the same with `mmnn_jpegll_decode` in front of each decode
`--parent_us`: the native_device_us of the parent build, measured in the same session with that build's own tools/dicom_ingest_time.py;
it is recorded beside this build's figure.  The host's share: parsing the 96 files of scan and mask in each syntax, `decode_series` as
a whole, and the numpy restatement (tests/_dicom_jpegll_ref.py) on one frame, times 48: what decodes such a series without this path."""
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
from dicom_rle_time import BOX, SHAPE, Staged as RleStaged  # noqa: E402
from dicom_timing import best_ms, decode, queued_us  # noqa: E402
from radiomics_time import ROTATING, copy_tbs, ellipsoid, kernel_split  # noqa: E402


class Staged:
    """A JPEG Lossless series on the device as `decode_series` stages it, with the buffers `mmnn_jpegll_decode` writes."""

    def __init__(self, series):
        x, y, z = series.shape
        starts = np.zeros(z + 1, dtype=np.int64)
        np.cumsum([(f.size + 15) // 16 * 16 for f in series.frames], out=starts[1:])
        payload = np.zeros(int(starts[-1]), dtype=np.uint8)
        records = np.zeros(z, dtype=ingest.JPEGLL_FRAME)
        for k, (f, scan) in enumerate(zip(series.frames, series.jpeg)):
            payload[starts[k]:starts[k] + f.size] = f
            records[k]["offset"], records[k]["length"], records[k]["precision"] = int(starts[k]) + scan.offset, scan.length, scan.precision
            records[k]["bits"] = scan.bits
            records[k]["huffval"][:len(scan.huffval)] = scan.huffval
        self.series, self.payload_bytes = series, int(payload.size)
        self.payload, self.records = torch.from_numpy(payload).to("cuda"), torch.from_numpy(records.view(np.uint8)).to("cuda")
        self.words = torch.empty(x * y * z * (series.bits_allocated // 8), dtype=torch.uint8, device="cuda")
        self.status = torch.empty(z, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(_lib.count("mmnn_jpegll_workspace_bytes", x, y, z, series.bits_allocated), dtype=torch.uint8, device="cuda")
        self.desc = _lib.JpegllDesc(x, y, z, series.bits_allocated, self.payload_bytes)

    def expand(self, stream):
        _lib.check(_lib.lib().mmnn_jpegll_decode(ctypes.byref(self.desc), self.payload.data_ptr(), self.records.data_ptr(), self.words.data_ptr(),
                                                 self.status.data_ptr(), self.ws.data_ptr(), stream), "mmnn_jpegll_decode")


def decode_times(series, native, steps, warmup, stream, tbs):
    """The figures of `mmnn_jpegll_decode` on one series; `native`: its uncompressed twin, whose bytes the words must equal."""
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
    native_bytes = sum(f.size for f in native.frames)
    res = {"decode_us": round(queued_us(lambda: one.expand(stream), steps), 1), "decode_rotating_us": round(queued_us(rotating, steps), 1),
           "decode_floor_us": round((one.payload_bytes + one.words.numel()) / (tbs * 1e12) * 1e6, 2),
           "uploaded_bytes_jpegll": one.payload_bytes + one.records.numel(), "uploaded_bytes_native": native_bytes,
           "compression_ratio": round(native_bytes / sum(f.size for f in series.frames), 3),
           "stuffed_zeros": int(sum(f.tobytes().count(b"\xff\x00") for f in series.frames)),
           "kernels_us": kernel_split(lambda: one.expand(stream))}
    return res, one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", type=str, default=os.path.join("profiles", "dicom_jpegll_time.json"))
    ap.add_argument("--decode_only", action="store_true", help="the decode figures alone (no RLE twin, no end-to-end run, no host share)")
    ap.add_argument("--parent_us", type=float, default=None, help="native_device_us of the parent build, measured in the same session")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    noise = rng.integers(-32768, 32768, SHAPE, dtype=np.int64).astype(np.int16)
    roi = ellipsoid()
    smooth = (roi.astype(np.int16) * 1000 + rng.integers(0, 16, SHAPE, dtype=np.int64).astype(np.int16))
    mask = np.zeros(SHAPE, dtype=np.uint8)
    (x0, y0, z0), (x1, y1, z1) = BOX
    mask[x0:x1, y0:y1, z0:z1] = 1
    voxels = int(np.prod(SHAPE))
    stream = torch.cuda.current_stream().cuda_stream
    tbs = copy_tbs(a.steps)
    with tempfile.TemporaryDirectory() as d:
        affine = np.diag([0.7, 0.7, 3.0, 1.0])
        path = lambda *p: os.path.join(d, *p)
        syntaxes = ("native", "jpeg-lossless") if a.decode_only else ("native", "rle", "jpeg-lossless")
        for syntax in syntaxes:
            synth_dicom.write_series(path(syntax, "image"), noise, affine, 0.25, -12.5, seed=1, transfer_syntax=syntax)
            synth_dicom.write_series(path(syntax, "mask"), mask * np.uint8(255), affine, seed=2, transfer_syntax=syntax)
            if syntax != "rle":
                synth_dicom.write_series(path(syntax, "smooth"), smooth, affine, 0.25, -12.5, seed=4, transfer_syntax=syntax)
                synth_dicom.write_series(path(syntax, "roi"), roi * np.uint8(255), affine, seed=3, transfer_syntax=syntax)
        read = lambda syntax, what, **kw: dicom.read_series(path(syntax, what), **kw)
        series = {(s, w): read(s, w) for s in ("native", "jpeg-lossless") for w in ("image", "mask", "smooth", "roi")}
        results = {}
        for name, what in (("noise_int16", "image"), ("smooth_int16", "smooth"), ("box_mask_uint8", "mask"), ("ellipsoid_mask_uint8", "roi")):
            results[name], staged = decode_times(series["jpeg-lossless", what], series["native", what], a.steps, a.warmup, stream, tbs)
            if what == "image":
                jll_s = staged
            if what == "mask":
                jll_m = staged
        head = {"shape": list(SHAPE), "steps": a.steps, "warmup": a.warmup, "copy_TBs": round(tbs, 2), "rotating_sets": ROTATING,
                **results}
        if a.decode_only:
            print(json.dumps(head), flush=True)
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(head, f, indent=1)
            return
        host = {f"parse_{s}_ms": best_ms(lambda: (read(s, "image"), read(s, "mask")), sync=True) for s in syntaxes}
        series.update({("rle", w): read("rle", w) for w in ("image", "mask")})
        for s in syntaxes:
            host[f"stage_upload_decode_{s}_ms"] = best_ms(lambda: (ingest.upload(series[s, "image"], "cuda"), ingest.upload(series[s, "mask"], "cuda")), sync=True)
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import _dicom_jpegll_ref as R
        j = series["jpeg-lossless", "image"]
        t = time.perf_counter()
        words, bad = R.decode_frame(j.frames[0][j.jpeg[0].offset:].tobytes(), j.jpeg[0].bits.tolist(), j.jpeg[0].huffval.tolist(), 16, SHAPE[0], SHAPE[1], 16)
        host["numpy_restatement_one_frame_s"] = round(time.perf_counter() - t, 2)
        host["numpy_restatement_volume_s"] = round(host["numpy_restatement_one_frame_s"] * SHAPE[2], 1)
        assert not bad and words.tobytes() == series["native", "image"].frames[0].tobytes()

        rle_s, rle_m = RleStaged(series["rle", "image"]), RleStaged(series["rle", "mask"])

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

        def compressed_volume(s, m):
            def run():
                s.expand(stream)
                m.expand(stream)
                behind(s.words, m.words)
            return run

        for _ in range(a.warmup):
            native_volume()
        torch.cuda.synchronize()
        kept, plane_n = ext.cpu().tolist(), plane.clone()
        for run in (compressed_volume(rle_s, rle_m), compressed_volume(jll_s, jll_m)):
            for _ in range(a.warmup):
                run()
            torch.cuda.synchronize()
            assert kept == ext.cpu().tolist() == [b - a_ for a_, b in zip(*BOX)] and torch.equal(plane_n, plane), (kept, ext)
        native_us = [queued_us(native_volume, a.steps) for _ in range(3)]
        rle_us = [queued_us(compressed_volume(rle_s, rle_m), a.steps) for _ in range(3)]
        jll_us = [queued_us(compressed_volume(jll_s, jll_m), a.steps) for _ in range(3)]
    res = {**head, "native_device_us": [round(v, 1) for v in native_us], "rle_device_us": [round(v, 1) for v in rle_us],
           "jpegll_device_us": [round(v, 1) for v in jll_us], "jpegll_minus_native_us": round(min(jll_us) - min(native_us), 1),
           "parent_build_native_device_us": a.parent_us, "host_per_volume": host}
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
