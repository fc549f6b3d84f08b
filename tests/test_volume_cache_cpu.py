"""`not gpu` tests of the volume cache's host side (mmnn_sts_amd/data/cache.py): the slot table and its counters, the capacity rule,
`CachedByUIDs` over a stub dataset and a stub cache, the binding of `mmnn_gather_rows` against the header, and the refusals of
`--cache_volumes` / `--cache_gb` in main.py."""
import ctypes
import os
import re

import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import cache as C
from mmnn_sts_amd.data.ingest import RawPatient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_table_first_come_and_full():
    t = C.SlotTable(3)
    assert [t.assign(u) for u in (1014, 1000, 1007)] == [0, 1, 2]
    assert t.assign(1000) == 1 and t.slot(1014) == 0 and len(t) == 3          # a uid keeps its slot
    assert t.assign(1021) is None and t.assign(1028) is None                   # full: no slot, and nobody loses theirs
    assert [t.slot(u) for u in (1014, 1000, 1007, 1021)] == [0, 1, 2, None]
    assert t.assign("1007") == 2                                               # (uids are compared as integers)
    for bad in (-1, 2.0, True, None):
        with pytest.raises(ValueError, match="capacity"):
            C.SlotTable(bad)
    empty = C.SlotTable(0)
    assert empty.assign(5) is None and empty.overflow == 1


def test_slot_table_filled_and_counters():
    t = C.SlotTable(2)
    assert not t.filled(7) and t.n_filled == 0
    assert t.assign(7) == 0 and not t.filled(7)                                # a slot is not filled before its owner says so
    with pytest.raises(KeyError):
        t.hit(7)
    t.mark_filled(7)
    assert t.filled(7) and t.filled("7") and t.n_filled == 1
    with pytest.raises(KeyError):
        t.mark_filled(8)                                                       # no slot to fill
    assert t.hit(7) == 0 and t.hit(7) == 0
    assert t.assign(9) == 1 and t.assign(11) is None and t.assign(11) is None
    assert (t.hits, t.misses, t.overflow) == (2, 2, 2)
    assert t.take_counters() == (2, 2, 2) and t.take_counters() == (0, 0, 0)
    assert t.filled(7) and t.slot(9) == 1                                      # the counters start again, the table does not


def test_capacity_for():
    gib = 2 ** 30
    assert C.row_bytes(2, 64) == 2 * 64 ** 3 * 4 + 24 == 2097176
    assert C.capacity_for(16 * gib, 2, 64, 10 ** 6) == 16 * gib // 2097176 == 8191             # "8000 patients at 2 x 64^3"
    assert C.capacity_for(16 * gib, 2, 128, 10 ** 6) == 16 * gib // (2 * 128 ** 3 * 4 + 24) == 1023   # "1000 at 2 x 128^3"
    assert C.capacity_for(2097175, 2, 64, 10) == 0                             # a budget below one row
    assert C.capacity_for(2097176, 2, 64, 10) == 1
    assert C.capacity_for(16 * gib, 2, 64, 300) == 300                         # fewer patients than the budget allows
    assert C.capacity_for(16 * gib, 1, 64, 0) == 0
    with pytest.raises(ValueError):
        C.capacity_for(gib, 0, 64, 3)


class _Dataset:
    """Counts `getDataByUID` calls; items as the image datasets (plain) or the multimodal ones ({'image', 'clinical'}) yield them."""

    def __init__(self, multimodal):
        self.uids, self.calls, self.multimodal = [1000, 1007, 1014], [], multimodal

    def getDataByUID(self, uid):
        self.calls.append(uid)
        raw = RawPatient(uid, [("scan", "mask")])
        x = {"image": raw, "clinical": torch.full((4,), float(uid))} if self.multimodal else raw
        return x, torch.tensor([uid % 2, 1]), torch.tensor([uid, uid + 1])


class _Cache:
    def __init__(self):
        self.have = set()

    def filled(self, uid):
        return uid in self.have


@pytest.mark.parametrize("multimodal", [False, True])
def test_cached_by_uids(multimodal):
    ds, cache = _Dataset(multimodal), _Cache()
    sub = C.CachedByUIDs(ds, [1014, 1000, 1007], cache)
    assert len(sub) == 3 and sub.uids == [1014, 1000, 1007]
    first = sub[0]
    image = first[0]["image"] if multimodal else first[0]
    assert ds.calls == [1014] and isinstance(image, RawPatient) and image.uid == 1014          # delegated, the item unchanged
    again = sub[0]
    assert ds.calls == [1014, 1014] and isinstance(again[0]["image"] if multimodal else again[0], RawPatient)   # not filled yet: delegated
    cache.have.add(1014)
    for _ in range(2):
        x, ev, du = sub[0]
        assert ds.calls == [1014, 1014]                                                         # no call: no file is opened
        assert (x["image"] if multimodal else x) == C.CachedPatient(1014)
        assert torch.equal(ev, first[1]) and torch.equal(du, first[2])
        if multimodal:
            assert set(x) == {"image", "clinical"} and torch.equal(x["clinical"], first[0]["clinical"])
    assert sub.getDataByUID(1014)[0] == x and ds.calls == [1014, 1014]
    # a uid that got no slot (overflow) never becomes filled: delegated every time
    for k in range(3):
        item = sub[1]
        assert isinstance(item[0]["image"] if multimodal else item[0], RawPatient) and ds.calls == [1014, 1014] + [1000] * (k + 1)
    # filled in the cache before this sub-dataset ever saw the uid (the validation set shares the cache): the first access is delegated
    cache.have.add(1007)
    assert isinstance((sub[2][0]["image"] if multimodal else sub[2][0]), RawPatient) and ds.calls[-1] == 1007
    n = len(ds.calls)
    assert (sub[2][0]["image"] if multimodal else sub[2][0]) == C.CachedPatient(1007) and len(ds.calls) == n


def test_gather_rows_binding_and_header():
    I, Q, V, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER
    restype, args = _lib._signatures()["mmnn_gather_rows"]
    assert restype is I and args == [V, Q, Q, P(I), I, V, V]
    header = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    proto = re.search(r"int\s+mmnn_gather_rows\s*\(([^)]*)\)\s*;", code)
    assert proto, "mmnn_gather_rows is not declared in include/mmnn_sts.h"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    assert params == ["const void* table", "int64_t n_rows", "int64_t row_bytes", "const int32_t* slots", "int32_t n", "void* out", "void* stream"]
    macro = re.search(r"^#define\s+MMNN_GATHER_MAX_ROWS\s+(\d+)\s*$", code, flags=re.M)
    assert macro and int(macro.group(1)) == _lib.GATHER_MAX_ROWS == 256
    assert os.path.exists(os.path.join(ROOT, "mmnn_sts_amd", "csrc", "gather.hip"))


def test_main_refuses_cache_flags(tmp_path, monkeypatch):
    import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    loc = ["--image_loc", str(tmp_path), "--key_loc", "k.csv", "--data_loc", "c.csv"]
    with pytest.raises(SystemExit, match=r"--cache_volumes keeps the ingested scans.*needs --image_loc"):
        main.main(["--images", "--survival", "--cache_volumes"])
    with pytest.raises(SystemExit, match=r"--cache_volumes.*--inference reads each patient once"):
        main.main(["--images", "--survival", "--inference", "--cache_volumes", *loc])
    with pytest.raises(SystemExit, match=r"--cache_volumes.*--lr_finder runs on synthetic patients"):
        main.main(["--images", "--classification", "--lr_finder", "--cache_volumes", *loc])
    for bad in ("0", "-2.5", "nan", "inf"):
        with pytest.raises(SystemExit, match=r"--cache_gb .* is not a positive number of GB"):
            main.main(["--images", "--survival", "--cache_volumes", "--cache_gb", bad, *loc])
    with pytest.raises(SystemExit, match=r"--cache_gb is the budget of the volume cache: it needs --cache_volumes"):
        main.main(["--images", "--survival", "--cache_gb", "4", *loc])
