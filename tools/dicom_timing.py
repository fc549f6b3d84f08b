"""What tools/dicom_ingest_time.py, tools/rtstruct_time.py and tools/seg_time.py share: the two timers and the bare kernel calls they
queue (no upload, no allocation), so the three measure one way."""
import ctypes
import time

import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import ingest


def queued_us(fn, steps):
    """Device time of one call in microseconds: `steps` calls queued back to back behind a spin kernel, between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(50_000_000)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def best_ms(fn, repeats=3, sync=False):
    """Best wall time of `repeats` calls in milliseconds; with `sync` the device is drained before and after each."""
    out = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        keep = fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
        del keep
    return round(min(out), 2)


def decode(series, pixels, out, stream):
    """`mmnn_decode_slices` alone: the slices' bytes already on the device (`pixels`) -> the volume in its integer type (`out`)."""
    desc = _lib.DecodeSlicesDesc(*series.shape, series.bits_allocated, series.bits_stored, series.high_bit, int(series.signed),
                                 ingest._integer_code(series.bits_allocated, series.signed))
    _lib.check(_lib.lib().mmnn_decode_slices(ctypes.byref(desc), pixels.data_ptr(), None, out.data_ptr(), stream), "mmnn_decode_slices")


def ingest_passes(scan, mask, plane, ext, ws, stream):
    """`mmnn_ingest_volume` alone, the three ingest passes, on two DeviceVolumes of one grid."""
    desc = _lib.IngestDesc(*scan.shape, scan.datatype, mask.datatype, scan.slope, scan.inter, mask.slope, mask.inter)
    _lib.check(_lib.lib().mmnn_ingest_volume(ctypes.byref(desc), scan.data.data_ptr(), mask.data.data_ptr(), plane.data_ptr(), ext.data_ptr(),
                                             ws.data_ptr(), stream), "mmnn_ingest_volume")
