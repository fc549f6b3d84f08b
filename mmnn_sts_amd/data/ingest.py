"""Raw scans -> the device batch: binding of `mmnn_ingest_volume` (csrc/ingest.hip) and the collate function built on it.

What upstream's NIfTI datasets do per patient and modality in `__getitem__` (data/ImageDatasets.py:431-470, :599-637: image * mask,
every all-zero slice dropped along each axis, Resize((64,64,64)), T1 / T2 stacked along the channel axis) runs here on the device, from
the file's voxels in their on-disk type.  The host only uploads bytes (pinned, non-blocking) and enqueues; it never waits.

    upload(volume, device)                          host volume (NiftiImage or ndarray) -> DeviceVolume
    ingest_volume(scan, mask, out_plane, extents)   one volume -> one 64^3 channel plane
    collate_volumes(patients, device)               [[(scan, mask) per modality] per patient] -> (N, C, 64,64,64) fp32, (N, C, 3) int32
    IngestCollate(device)                           the DataLoader collate_fn of the NIfTI datasets
"""
import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .nifti import NiftiImage

SIZE = 64                                    # MMNN_INGEST_SIZE
TYPE_CODES = {np.dtype("uint8"): 2, np.dtype("int16"): 4, np.dtype("int32"): 8, np.dtype("float32"): 16, np.dtype("float64"): 64,
              np.dtype("int8"): 256, np.dtype("uint16"): 512, np.dtype("uint32"): 768}


@dataclass
class DeviceVolume:
    """A scan's voxels on the device as the file holds them: `data` is a flat uint8 tensor of x*y*z elements of NIfTI type `datatype`,
    x fastest."""
    data: torch.Tensor
    shape: Tuple[int, int, int]
    datatype: int
    slope: float = 1.0
    inter: float = 0.0


@dataclass
class RawPatient:
    """What a NIfTI dataset's `__getitem__` yields in place of a float volume: per modality the (scan, mask) pair, still raw."""
    uid: int
    volumes: List[Tuple[NiftiImage, NiftiImage]]


def _host_bytes(raw: np.ndarray) -> np.ndarray:
    """The volume's bytes with x fastest, without a copy when the array already is x-fastest (as the reader returns it)."""
    if raw.ndim != 3:
        raise ValueError(f"ingest: a volume has three axes, got an array of shape {raw.shape}")
    if raw.dtype not in TYPE_CODES:
        raise ValueError(f"ingest: dtype {raw.dtype} has no supported NIfTI type code ({sorted(str(k) for k in TYPE_CODES)})")
    return np.ascontiguousarray(raw.T).reshape(-1).view(np.uint8)


def upload(volume, device, slope: float = 1.0, inter: float = 0.0) -> DeviceVolume:
    """Host -> device, in the on-disk type.  `volume`: a NiftiImage (its slope / inter are used) or an (x, y, z) ndarray."""
    if isinstance(volume, DeviceVolume):
        return volume
    if isinstance(volume, NiftiImage):
        raw, slope, inter = volume.raw, volume.slope, volume.inter
    else:
        raw = np.asarray(volume)
    if not raw.dtype.isnative:
        raw = raw.astype(raw.dtype.newbyteorder("="))
    host = torch.from_numpy(_host_bytes(raw)).pin_memory()
    return DeviceVolume(host.to(device, non_blocking=True), tuple(int(s) for s in raw.shape), TYPE_CODES[raw.dtype], float(slope), float(inter))


def workspace_bytes(x: int, y: int, z: int) -> int:
    n = _lib.lib().mmnn_ingest_workspace_bytes(int(x), int(y), int(z))
    if n < 0:
        raise ValueError("mmnn_ingest_workspace_bytes: " + _lib.last_error())
    return int(n)


def ingest_volume(scan, mask, out_plane: torch.Tensor, extents: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Enqueue the ingest of one volume on the current stream: `out_plane` (a contiguous (64,64,64) fp32 CUDA view, e.g. batch[n, c]) receives
    the masked, compacted, area-resized scan; returns `extents` (3 x int32 on the device: kept slices along x, y, z), readable after
    the next synchronisation.  `scan` / `mask`: DeviceVolume, NiftiImage or ndarray (host volumes are uploaded first)."""
    if not (out_plane.is_cuda and out_plane.dtype == torch.float32 and out_plane.is_contiguous() and tuple(out_plane.shape) == (SIZE,) * 3):
        raise ValueError(f"ingest: out_plane must be a contiguous ({SIZE},{SIZE},{SIZE}) fp32 CUDA tensor, got {tuple(out_plane.shape)} {out_plane.dtype} on {out_plane.device}")
    dev = out_plane.device
    scan, mask = upload(scan, dev), upload(mask, dev)
    if scan.shape != mask.shape:
        raise ValueError(f"ingest: scan extent {scan.shape} differs from the mask's {mask.shape}")
    if extents is None:
        extents = torch.empty(3, dtype=torch.int32, device=dev)
    if not (extents.is_cuda and extents.dtype == torch.int32 and extents.is_contiguous() and extents.numel() == 3):
        raise ValueError("ingest: extents must be 3 contiguous int32 on the device")
    x, y, z = scan.shape
    nbytes = workspace_bytes(x, y, z)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError(f"ingest: workspace of {workspace.numel() * workspace.element_size()} bytes, {nbytes} needed")
    desc = _lib.IngestDesc(x, y, z, scan.datatype, mask.datatype, scan.slope, scan.inter, mask.slope, mask.inter)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mmnn_ingest_volume(ctypes.byref(desc), scan.data.data_ptr(), mask.data.data_ptr(), out_plane.data_ptr(),
                                                 extents.data_ptr(), workspace.data_ptr(), stream), "mmnn_ingest_volume")
    return extents


def collate_volumes(patients: Sequence[Sequence[Tuple[object, object]]], device) -> Tuple[torch.Tensor, torch.Tensor]:
    """patients[n][c] = (scan, mask) -> the device batch (N, C, 64, 64, 64) fp32 and the kept extents (N, C, 3) int32.  Every upload is
    issued before the first kernel, so the copies of one volume run beside the passes of the one before it."""
    n, c = len(patients), len(patients[0])
    if any(len(p) != c for p in patients):
        raise ValueError("ingest: patients of one batch differ in their number of modalities")
    device = torch.device(device)
    up = [[(upload(s, device), upload(m, device)) for s, m in p] for p in patients]
    batch = torch.empty((n, c, SIZE, SIZE, SIZE), dtype=torch.float32, device=device)
    extents = torch.empty((n, c, 3), dtype=torch.int32, device=device)
    for i in range(n):
        for j in range(c):
            ingest_volume(up[i][j][0], up[i][j][1], batch[i, j], extents[i, j])
    return batch, extents


class IngestCollate:
    """collate_fn of the NIfTI datasets: items are (x, events, durations) or (x, labels) with x a RawPatient or
    {'image': RawPatient, 'clinical': tensor}; returns (x, events, durations) (durations None for classification items) with the image
    batch on `device`.  The extents of every batch are kept in `pending` until `take_empty()` reads them: call it where the epoch
    synchronises anyway, never per batch."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.pending: List[Tuple[List[int], torch.Tensor]] = []

    def __call__(self, items):
        xs = [it[0] for it in items]
        targets = [torch.stack([torch.as_tensor(it[k]) for it in items]) for k in range(1, len(items[0]))]
        multimodal = isinstance(xs[0], dict)
        raws = [x["image"] for x in xs] if multimodal else xs
        batch, extents = collate_volumes([r.volumes for r in raws], self.device)
        self.pending.append(([r.uid for r in raws], extents))
        x = {"image": batch, "clinical": torch.stack([x["clinical"] for x in xs]).float()} if multimodal else batch
        return (x, targets[0], targets[1] if len(targets) > 1 else None)

    def take_empty(self) -> List[int]:
        """uids (sorted, each once) of the patients seen since the last call whose mask left nothing of a scan (an extent of 0)."""
        bad = set()
        for uids, ext in self.pending:
            hit = (ext.cpu() == 0).any(dim=2).any(dim=1).tolist()
            bad.update(u for u, h in zip(uids, hit) if h)
        self.pending = []
        return sorted(bad)
