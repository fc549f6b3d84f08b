"""GPU tests of the volume cache: `mmnn_gather_rows` (csrc/gather.hip) against `table.cpu()[slots]` as int32 bit patterns, with the output
carved out of a larger buffer whose sentinel dwords on both sides must survive; `IngestCollate(cache=)` + `CachedByUIDs` against the
uncached collate on the same items, bit for bit, with the file reader disabled in the cached pass; and `main.py --cache_volumes` in fresh
processes."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import cache as C
from mmnn_sts_amd.data import ingest, nifti, synth_dicom, synth_nifti
from mmnn_sts_amd.data.ImageDatasets import ImageDataset, ImageDatasetByUIDs, T1T2SurvivalDataset
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                   # sentinel dwords on each side of `out` (256 bytes: `out` keeps the allocation's alignment)
SENTINEL = 0x5A5A1234


def _patterns(n_rows, dwords, seed, shift=0):
    """(n_rows, dwords) random 32-bit patterns on the device, starting 4 * shift bytes into their allocation."""
    host = torch.from_numpy(np.random.default_rng(seed).integers(0, 2 ** 32, size=n_rows * dwords + shift, dtype=np.uint32).view(np.int32))
    return host.to(DEV)[shift:].view(n_rows, dwords)


def _carve(n, dwords, shift=0):
    """(the whole buffer, `out` (n, dwords) inside it starting GUARD + shift dwords in), everything filled with the sentinel."""
    buf = torch.full((2 * GUARD + n * dwords + shift,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD + shift:GUARD + shift + n * dwords].view(n, dwords)


def _guards_intact(buf, out):
    lead = (out.data_ptr() - buf.data_ptr()) // 4
    host = buf.cpu()
    return bool((host[:lead] == SENTINEL).all()) and bool((host[lead + out.numel():] == SENTINEL).all()) and lead >= GUARD


def _check_gather(table, slots, out_shift=0):
    buf, out = _carve(len(slots), table.shape[1], out_shift)
    C.gather_rows(table, slots, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), table.cpu()[torch.tensor(slots)])
    assert _guards_intact(buf, out)


@pytest.mark.parametrize("row_bytes", [4, 12, 24, 108, 256, 4096, 2097152])
def test_gather_row_sizes(row_bytes):
    """4, 12, 24 and 108 take the dword path, the others the 16-byte path."""
    table = _patterns(7, row_bytes // 4, row_bytes)
    assert table.data_ptr() % 16 == 0
    _check_gather(table, [6, 0, 3, 3, 5])


@pytest.mark.parametrize("row_bytes", [256, 4096])
@pytest.mark.parametrize("shifted", ["table", "out"])
def test_gather_forced_dword_path(row_bytes, shifted):
    """Sizes that could go by 16 bytes, with one side 4 bytes off a 16-byte boundary."""
    table = _patterns(7, row_bytes // 4, row_bytes + 1, shift=1 if shifted == "table" else 0)
    assert table.data_ptr() % 16 == (4 if shifted == "table" else 0)
    _check_gather(table, [6, 0, 3, 3, 5], out_shift=1 if shifted == "out" else 0)


@pytest.mark.parametrize("n", [1, 256, 300])
def test_gather_row_counts(n):
    """n = 1, n = MMNN_GATHER_MAX_ROWS in one launch, and 300 rows in two chunks."""
    assert _lib.GATHER_MAX_ROWS == 256
    table = _patterns(300, 64, n)
    slots = np.random.default_rng(n).integers(0, 300, size=n).tolist()
    _check_gather(table, slots)


def test_gather_offsets_beyond_32_bits():
    """260 rows of 16 MiB: row 256 starts at byte 2^32, so a 32-bit offset would read rows 0 and 3 for 256 and 259."""
    row = 16 << 20
    table = torch.empty(260 * row, dtype=torch.uint8, device=DEV).view(torch.int32).view(260, row // 4)
    base = torch.arange(row // 4, dtype=torch.int32, device=DEV)
    for r in (0, 255, 256, 259):
        table[r] = base ^ (r * 0x01010101 + 0x00F00000)
    slots = [259, 256, 255, 0]
    buf, out = _carve(4, row // 4)
    C.gather_rows(table, slots, out)
    torch.cuda.synchronize()
    for i, r in enumerate(slots):
        assert torch.equal(out[i], base ^ (r * 0x01010101 + 0x00F00000)), f"out row {i} is not table row {r}"
    assert _guards_intact(buf, out)


def test_gather_refusals():
    """Every refusal of the header comment: a ValueError that names the argument, raised by host checks, so nothing is launched."""
    table = _patterns(7, 64, 5)
    buf, out = _carve(5, 64)
    t, o, stream = table.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream

    def call(table=t, n_rows=7, row_bytes=256, slots=(6, 0, 3, 3, 5), n=None, out=o):
        arr = None if slots is None else (ctypes.c_int32 * max(1, len(slots)))(*slots)
        _lib.call("mmnn_gather_rows", table, n_rows, row_bytes, arr, len(slots) if n is None else n, out, stream)

    for kw, message in (({"table": None}, "table is null"), ({"slots": None, "n": 5}, "slots is null"), ({"out": None}, "out is null"),
                        ({"n_rows": 0}, "n_rows 0"), ({"n_rows": -3}, "n_rows -3"), ({"row_bytes": 0}, "row_bytes 0"),
                        ({"row_bytes": 2}, "row_bytes 2"), ({"row_bytes": 254}, "row_bytes 254"), ({"row_bytes": -4}, "row_bytes -4"),
                        ({"n": 0}, "n 0 outside 1..256"), ({"slots": (0,) * 257}, "n 257 outside 1..256"), ({"n": -1}, "n -1 outside"),
                        ({"slots": (6, -1, 3)}, r"slots\[1\] = -1"), ({"slots": (6, 0, 7)}, r"slots\[2\] = 7 outside 0\.\.6"),
                        ({"table": t + 2}, "table not aligned"), ({"out": o + 2}, "out not aligned"),
                        ({"out": t + 256}, "out overlaps the table"), ({"out": t + 6 * 256}, "out overlaps the table"),
                        ({"table": o + 256, "n_rows": 1, "slots": (0,) * 5}, "out overlaps the table")):
        with pytest.raises(ValueError, match="mmnn_gather_rows: gather_rows: " + message):
            call(**kw)
    call(out=o)                                                                 # the same call, accepted
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), table.cpu()[torch.tensor([6, 0, 3, 3, 5])]) and _guards_intact(buf, out)
    with pytest.raises(ValueError, match="out must hold 2 >= 1 rows of 256 bytes"):
        C.gather_rows(table, [1, 2], out)


# ---- the collate with a cache against the collate without one ---------------------------------------------------------------------------
PASS_1, PASS_2 = ([0, 1], [2, 3], [4]), ([3, 0], [4, 2], [1])


def _dataset(tree):
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])


def _collated(collate, sub, indices):
    """(batch, extents, events, durations) of the items `indices` of `sub`."""
    x, ev, du = collate([sub[i] for i in indices])
    return x, collate.pending[-1][1], ev, du


def _reference(ds, size, batches, **kw):
    plain, collate = ImageDatasetByUIDs(ds, ds.uids), ingest.IngestCollate(DEV, size=size, **kw)
    want = {tuple(b): _collated(collate, plain, b) for b in batches}
    torch.cuda.synchronize()
    return want


def _assert_same(got, want, what):
    torch.cuda.synchronize()
    for g, w, name in zip(got, want, ("batch", "extents", "events", "durations")):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), f"{what}: {name} differs"


def _no_reading(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a file was read for a patient the cache holds")
    monkeypatch.setattr(nifti, "read", refuse)


@pytest.mark.parametrize("size", [8, 64])
def test_cached_collate_equals_uncached(tmp_path, monkeypatch, size):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=5, seed=61)
    ds = _dataset(tree)
    want = _reference(ds, size, PASS_1 + PASS_2)
    cache = C.VolumeCache(DEV, 2, size, 5)
    collate = ingest.IngestCollate(DEV, size=size, cache=cache)
    sub = C.CachedByUIDs(ds, ds.uids, cache)
    for b in PASS_1:
        _assert_same(_collated(collate, sub, b), want[tuple(b)], f"pass 1, batch {b}")
    assert cache.table.take_counters() == (0, 5, 0) and cache.table.n_filled == 5 and cache.bytes_held == 5 * C.row_bytes(2, size)
    _no_reading(monkeypatch)
    for b in PASS_2:
        assert all(isinstance(sub[i][0], C.CachedPatient) for i in b)
        _assert_same(_collated(collate, sub, b), want[tuple(b)], f"pass 2, batch {b}")
    assert cache.table.take_counters() == (5, 0, 0)
    assert float(want[(0, 1)][0].abs().max()) > 0.0 and int(want[(0, 1)][1].min()) > 0
    assert collate.take_empty() == []


def test_overflow_patients_are_read_every_time(tmp_path, monkeypatch):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=5, seed=62)
    ds = _dataset(tree)
    want = _reference(ds, 8, PASS_1 + PASS_2)
    cache = C.VolumeCache(DEV, 2, 8, 3)
    collate = ingest.IngestCollate(DEV, size=8, cache=cache)
    sub = C.CachedByUIDs(ds, ds.uids, cache)
    ImageDataset.files_read = 0
    for b in PASS_1:
        _assert_same(_collated(collate, sub, b), want[tuple(b)], f"pass 1, batch {b}")
    assert ImageDataset.files_read == 5 * 4                                      # two modalities, a scan and a mask each
    assert cache.table.take_counters() == (0, 3, 2) and cache.table.n_filled == 3
    read, ImageDataset.files_read = [], 0
    real = nifti.read
    monkeypatch.setattr(nifti, "read", lambda path, *a, **k: (read.append(str(path)), real(path, *a, **k))[1])
    for b in PASS_2:
        _assert_same(_collated(collate, sub, b), want[tuple(b)], f"pass 2, batch {b}")
    assert cache.table.take_counters() == (3, 0, 2)
    assert ImageDataset.files_read == 2 * 4 == len(read)                         # exactly the two patients without a slot
    assert {os.path.basename(os.path.dirname(p))[:8] for p in read} == {"SYN-0003", "SYN-0004"}


def test_mask_on_its_own_grid(tmp_path, monkeypatch):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=63, mask_grid="own")
    ds = _dataset(tree)
    assert len(ds.t1_dataset.other_grid) == 3
    want = _reference(ds, 8, ([0, 1, 2],))[(0, 1, 2)]
    cache = C.VolumeCache(DEV, 2, 8, 3)
    collate = ingest.IngestCollate(DEV, size=8, cache=cache)
    sub = C.CachedByUIDs(ds, ds.uids, cache)
    _assert_same(_collated(collate, sub, [0, 1, 2]), want, "cold pass")
    _no_reading(monkeypatch)
    _assert_same(_collated(collate, sub, [0, 1, 2]), want, "cached pass")
    assert int(want[1].min()) > 0


def test_empty_mask_is_cached_and_reported_again(tmp_path, monkeypatch):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=3, seed=64, empty_mask_uids=(1007,))
    ds = _dataset(tree)
    want = _reference(ds, 8, ([0, 1, 2],))[(0, 1, 2)]
    cache = C.VolumeCache(DEV, 2, 8, 3)
    collate = ingest.IngestCollate(DEV, size=8, cache=cache)
    sub = C.CachedByUIDs(ds, ds.uids, cache)
    _assert_same(_collated(collate, sub, [0, 1, 2]), want, "cold pass")
    assert collate.take_empty() == [1007]
    _no_reading(monkeypatch)
    _assert_same(_collated(collate, sub, [2, 1, 0]), tuple(t.flip(0) for t in want), "cached pass")
    assert collate.take_empty() == [1007] and collate.take_empty() == []
    assert float(want[0][1].abs().max()) == 0.0                                   # cached as the zeros the ingest wrote


def test_dicom_twin_gives_the_same_cached_batches(tmp_path):
    ntree = synth_nifti.write_tree(tmp_path / "nifti", n_patients=2, seed=21)
    dtree = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / "dicom", mask_value=255, shuffle_names=True, seed=21)
    got = {}
    for name, tree, threshold in (("nifti", ntree, 0.5), ("dicom", dtree, None)):
        ds = _dataset(tree)
        assert ds.layout == name
        cache = C.VolumeCache(DEV, 2, 64, 2)
        collate = ingest.IngestCollate(DEV, mask_threshold=threshold, cache=cache)
        sub = C.CachedByUIDs(ds, ds.uids, cache)
        cold = _collated(collate, sub, [0, 1])
        got[name] = _collated(collate, sub, [0, 1])
        _assert_same(got[name], cold, f"{name}: cached against cold")
        assert cache.table.take_counters() == (2, 2, 0)
    _assert_same(got["dicom"], got["nifti"], "the DICOM twin's cached batch against the NIfTI tree's")
    assert int(got["nifti"][1].min()) > 0


def test_keep_workspaces_excludes_a_cache():
    cache = C.VolumeCache(DEV, 2, 8, 1)
    with pytest.raises(ConfigurationError, match="keep_workspaces"):
        ingest.IngestCollate(DEV, size=8, keep_workspaces=True, cache=cache)
    with pytest.raises(ConfigurationError, match=r"8\^3 planes"):
        ingest.IngestCollate(DEV, size=16, cache=cache)


# ---- main.py ---------------------------------------------------------------------------------------------------------------------------
_main = functools.partial(run_main, limit_s=600)


CACHE_LINE = re.compile(r"volume cache: (\d+) of (\d+) patients cached, ([\d.]+) MB held; this epoch: (\d+) hits, (\d+) misses, (\d+) overflow, "
                        r"(\d+) files read")


def test_cli_two_epochs_with_a_cache(tmp_path):
    """Epoch 1 reads every patient's four files (T1 and T2, a scan and a mask each) and hits nothing; epoch 2 reads none.  The
    checkpoint is the uncached run's, tensor for tensor: two uncached runs of this command were identical on the device."""
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=4, seed=41, val_fraction=0.5)
    cfg = tiny_config(tmp_path)
    args = ["--images", "--preop", "--survival", "--blend", "--transforms", "--epochs", "2", "--config", cfg,
            "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
            "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]
    log = _main([*args, "--cache_volumes"], tmp_path / "cached")
    assert "epoch 2/2" in log and os.path.exists(tmp_path / "cached" / "best_surv_model.pth"), log[-2000:]
    lines = [tuple(float(v) if "." in v else int(v) for v in m.groups()) for m in CACHE_LINE.finditer(log)]
    patients = 4                                                                  # two to train on, two to validate on
    assert len(lines) == 2, log[-2000:]
    assert lines[0] == (patients, patients, round(patients * C.row_bytes(2, 64) / 1e6, 1), 0, patients, 0, 4 * patients)
    assert lines[1] == (patients, patients, round(patients * C.row_bytes(2, 64) / 1e6, 1), patients, 0, 0, 0)
    plain = _main(args, tmp_path / "plain")
    assert "volume cache" not in plain
    a, b = (torch.load(tmp_path / d / "best_surv_model.pth", map_location="cpu") for d in ("cached", "plain"))
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between the cached and the uncached run"
