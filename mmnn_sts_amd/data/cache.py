"""Ingested volumes kept on the device across epochs (`--cache_volumes`).

What the ingest makes of a patient is fixed -- it runs before `--transforms`, and two ingests of one (scan, mask) pair are bit-identical --
and small: C * S^3 floats, 2 MB at 2 x 64^3.  Reading the patient is not: gunzip and parse of the files cost the host three orders of
magnitude more than the device spends on them.  So each patient is read and ingested once, its S^3 planes and kept extents stay in one
row of a table on the device, and every later batch is assembled from those rows (`mmnn_gather_rows`, csrc/gather.hip) with no file opened.

    SlotTable(capacity)                                   uid -> row, first come first served, never reassigned; the counters
    capacity_for(budget_bytes, channels, size, n)         rows that fit the budget, at most n
    VolumeCache(device, channels, size, capacity)         the planes (capacity, C, S, S, S) fp32, the extents (capacity, C, 3) int32, a SlotTable
    VolumeCache.gather(slots, out_batch, out_extents)     rows -> a batch, on the current stream
    CachedPatient(uid)                                    stands in a loader item where a RawPatient would be
    CachedByUIDs(dataset, uids, cache)                    ImageDatasetByUIDs that stops calling the dataset for a patient the cache holds

`IngestCollate(..., cache=)` (`mmnn_sts_amd.data.ingest`) fills the rows and assembles the batches.  A patient that arrives when every
row is taken (overflow) is read and ingested every time, as without a cache.  The first epoch, inference and overflow patients still pay
the files; reading ahead with host threads and a cache on disk between runs are outside this module.
"""
import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from .. import _lib
from .ImageDatasets import ImageDatasetByUIDs

EXTENT_BYTES = 12                             # three int32 per channel


class SlotTable:
    """uid -> slot in first-come order.  A slot is never reassigned and a uid keeps the one it got; `assign` returns None once all are
    taken.  A slot is `filled` once its owner says so (`mark_filled`: the ingest into it has been enqueued).  Counters, since the last
    `take_counters`: `hits` (a filled slot served a patient), `misses` (a patient was ingested into a slot), `overflow` (a patient
    found no slot)."""

    def __init__(self, capacity: int):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0:
            raise ValueError(f"SlotTable: capacity must be a non-negative integer, got {capacity!r}")
        self.capacity = capacity
        self.slots: Dict[int, int] = {}
        self._filled = set()
        self.hits = self.misses = self.overflow = 0

    def __len__(self):
        return len(self.slots)

    def assign(self, uid) -> Optional[int]:
        """The slot of `uid`, a new one when it has none yet (counted as a miss); None when the table is full (counted as overflow)."""
        uid = int(uid)
        slot = self.slots.get(uid)
        if slot is None:
            if len(self.slots) >= self.capacity:
                self.overflow += 1
                return None
            slot = self.slots[uid] = len(self.slots)
        self.misses += 1
        return slot

    def slot(self, uid) -> Optional[int]:
        return self.slots.get(int(uid))

    def mark_filled(self, uid) -> None:
        if int(uid) not in self.slots:
            raise KeyError(f"SlotTable: uid {uid} has no slot to fill")
        self._filled.add(int(uid))

    def filled(self, uid) -> bool:
        return int(uid) in self._filled

    @property
    def n_filled(self) -> int:
        return len(self._filled)

    def hit(self, uid) -> int:
        """The slot of a filled `uid`, counted as a hit."""
        if not self.filled(uid):
            raise KeyError(f"SlotTable: uid {uid} is not filled")
        self.hits += 1
        return self.slots[int(uid)]

    def take_counters(self):
        """(hits, misses, overflow) since the last call; they start again at 0."""
        out = (self.hits, self.misses, self.overflow)
        self.hits = self.misses = self.overflow = 0
        return out


def row_bytes(channels: int, size: int) -> int:
    """What one patient occupies: C * S^3 floats and C kept-extent triples."""
    return channels * size ** 3 * 4 + channels * EXTENT_BYTES


def capacity_for(budget_bytes: int, channels: int, size: int, n_patients: int) -> int:
    """Rows that fit `budget_bytes`, at most `n_patients` (0: a budget below one row)."""
    if channels < 1 or size < 1:
        raise ValueError(f"capacity_for: channels {channels} and size {size} must be positive")
    return max(0, min(int(n_patients), int(budget_bytes) // row_bytes(channels, size)))


class VolumeCache:
    """The device side: `planes` (capacity, C, S, S, S) fp32 and `extents` (capacity, C, 3) int32, row = slot, and the `SlotTable`
    that says whose row it is.  The rows are written by the ingest itself (`IngestCollate(cache=)`) and read by `gather`."""

    def __init__(self, device, channels: int, size: int, capacity: int):
        self.channels, self.size = int(channels), int(size)
        self.table = SlotTable(capacity)
        device = torch.device(device)
        self.planes = torch.empty((capacity, self.channels, self.size, self.size, self.size), dtype=torch.float32, device=device)
        self.extents = torch.empty((capacity, self.channels, 3), dtype=torch.int32, device=device)

    @property
    def capacity(self) -> int:
        return self.table.capacity

    def filled(self, uid) -> bool:
        return self.table.filled(uid)

    @property
    def bytes_held(self) -> int:
        return self.table.n_filled * row_bytes(self.channels, self.size)

    def gather(self, slots: Sequence[int], out_batch: torch.Tensor, out_extents: torch.Tensor) -> None:
        """out_batch[i] = planes[slots[i]], out_extents[i] = extents[slots[i]], bit for bit, enqueued on the current stream: two
        `mmnn_gather_rows` calls, and two more per further `GATHER_MAX_ROWS` rows.  `out_batch`: contiguous (n, C, S, S, S) fp32,
        `out_extents`: contiguous (n, C, 3) int32, on the cache's device.  A slot outside the table is a ValueError of the library."""
        n = len(slots)
        dev = self.planes.device
        _lib.device_buffer(out_batch, (n,) + tuple(self.planes.shape[1:]), torch.float32, dev, "VolumeCache.gather (out_batch)")
        _lib.device_buffer(out_extents, (n,) + tuple(self.extents.shape[1:]), torch.int32, dev, "VolumeCache.gather (out_extents)")
        for table, out in ((self.planes, out_batch), (self.extents, out_extents)):
            gather_rows(table, slots, out)


def gather_rows(table: torch.Tensor, slots: Sequence[int], out: torch.Tensor) -> torch.Tensor:
    """Enqueue `mmnn_gather_rows` on the current stream of the table's device: out[i] = table[slots[i]] as bit patterns, for two
    contiguous device tensors whose rows (everything behind the first axis) hold the same number of bytes, a multiple of 4.  In
    chunks of `GATHER_MAX_ROWS` rows.  The checks of the slots and pointers are the library's (ValueError)."""
    n_rows, n = int(table.shape[0]), len(slots)
    if not (table.is_cuda and out.is_cuda and table.device == out.device and table.is_contiguous() and out.is_contiguous()):
        raise ValueError(f"gather_rows: table and out must be contiguous tensors of one GPU, got {table.device} and {out.device}")
    width = table[0].numel() * table.element_size() if n_rows else 0
    if int(out.shape[0]) != n or n < 1 or out[0].numel() * out.element_size() != width:
        raise ValueError(f"gather_rows: out must hold {n} >= 1 rows of {width} bytes, got {tuple(out.shape)} {out.dtype}")
    for at in range(0, n, _lib.GATHER_MAX_ROWS):
        part = [int(s) for s in slots[at:at + _lib.GATHER_MAX_ROWS]]
        _lib.enqueue("mmnn_gather_rows", table.data_ptr(), n_rows, width, (ctypes.c_int32 * len(part))(*part), len(part),
                     out.data_ptr() + at * width, device=table.device)
    return out


@dataclass
class CachedPatient:
    """Stands in a loader item where a `RawPatient` would be: the patient's planes are in the cache, no file was read."""
    uid: int


class CachedByUIDs(ImageDatasetByUIDs):
    """`ImageDatasetByUIDs` in front of a cache (anything with `filled(uid)`).  The first access of a uid goes to the dataset as ever,
    and the host part of its item is remembered: the targets, and x['clinical'] of a multimodal item -- a few floats.  Once the
    cache holds the uid the remembered item is returned with `CachedPatient(uid)` in the image's place and the dataset is not
    called, so no file is opened.  A uid that got no slot goes to the dataset every time."""

    def __init__(self, dataset, uids, cache, seed=42, train_percent=0.8, transforms=None):
        super().__init__(dataset, uids, seed, train_percent, transforms)
        self.cache = cache
        self._host_part = {}

    def getDataByUID(self, uid):
        uid = int(uid)
        if uid in self._host_part and self.cache.filled(uid):
            return self._host_part[uid]
        item = self.dataset.getDataByUID(uid)
        if uid not in self._host_part:
            stand_in = CachedPatient(uid)
            x = item[0]
            x = {k: (stand_in if k == self.multimodal_identifier else v) for k, v in x.items()} if isinstance(x, dict) else stand_in
            self._host_part[uid] = (x, *item[1:])
        return item

    def __getitem__(self, index):
        return self.getDataByUID(self.set_uids[index])
