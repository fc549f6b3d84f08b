"""Occlusion sensitivity on the MI355X (csrc/occlusion.hip, utils.OcclusionSensitivity, `main.py --occlusion`) against the numpy restatement
of its contract (tests/_occlusion_ref.py).  Everything here is exact: the occluded batches are compared as bit patterns, the maps with
array equality (the fp64 order is part of the contract and the library is built without FMA contraction), the channel means against the
two fp32 neighbours of the fp64 mean.  The real models are compared with their own eval() forward run on restated batches of the same
composition, so that both sides select the same kernels."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import _occlusion_ref as O
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FC0BEEF                      # a NaN pattern no input holds
GRID_A = ((2, 9, 10, 13), (4, 3, 5), (2, 3, 4))           # odd extents, clamped last windows, w = 13: the dword variant
GRID_B = ((2, 8, 8, 16), (4, 4, 8), (4, 2, 4))            # w % 4 == 0: the 16-byte variant


def _lib():
    from mmnn_sts_amd import _lib
    return _lib, _lib.lib()


def _desc(shape, win, stride):
    M, _ = _lib()
    return M.OcclusionDesc(*shape, (ctypes.c_int32 * 3)(*O.triple(win)), (ctypes.c_int32 * 3)(*O.triple(stride)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _input(shape, seed):
    """fp32 noise with NaNs (one with a payload), infinities and -0.0 planted in it."""
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    flat[3], flat[flat.size // 2], flat[-2] = 0x7FC00000, 0xFFC12345, 0x80000000
    flat[7], flat[flat.size // 3] = 0x80000000, 0x7F800000
    return x


def _occlude(x, fill, win, stride, first, count, lead):
    """The device batch as uint32 (count, c, d, h, w); `out` sits `lead` floats into a sentinel-filled buffer, whose other words must keep
    their value."""
    M, L = _lib()
    n = count * x.size
    buf = torch.full((lead + n + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    dx, dfill = torch.from_numpy(x).to(DEV), torch.from_numpy(np.asarray(fill, dtype=np.float32)).to(DEV)
    M.check(L.mmnn_occlude_windows(ctypes.byref(_desc(x.shape, win, stride)), dx.data_ptr(), dfill.data_ptr(), first, count,
                                   buf.data_ptr() + 4 * lead, _stream()), "mmnn_occlude_windows")
    torch.cuda.synchronize()
    b = buf.cpu().numpy().view(np.uint32)
    assert (b[:lead] == SENTINEL).all() and (b[lead + n:] == SENTINEL).all(), "words outside `out` were written"
    assert np.array_equal(dx.cpu().numpy().view(np.uint32), x.view(np.uint32)), "x was written"
    return b[lead:lead + n].reshape((count,) + x.shape)


def _wn(grid):
    return O.grid(grid[0][1:], grid[1], grid[2])[2]


# ---- mmnn_occlude_windows ---------------------------------------------------------------------------------------------------------------
_OCCLUDE_CASES = {
    "A all windows": (GRID_A, 0, _wn(GRID_A), 5), "A first 5 count 7": (GRID_A, 5, 7, 8), "A past Wn": (GRID_A, _wn(GRID_A) - 3, 8, 1),
    "A count 1": (GRID_A, 17, 1, 0),
    "B all windows": (GRID_B, 0, _wn(GRID_B), 8), "B first 5 count 7": (GRID_B, 5, 7, 16), "B past Wn": (GRID_B, _wn(GRID_B) - 3, 8, 4),
    "B count 1": (GRID_B, 11, 1, 0),
    "B out off the 16-byte grid": (GRID_B, 5, 7, 3),                                      # w % 4 == 0 and the dword variant all the same
    "A single window": ((GRID_A[0], GRID_A[0][1:], (1, 2, 3)), 0, 3, 2), "B single window": ((GRID_B[0], GRID_B[0][1:], (8, 8, 16)), 0, 1, 4),
    "A window 1": ((GRID_A[0], 1, 1), 1100, 90, 1), "B window 1": ((GRID_B[0], 1, 1), 1000, 40, 4),
    "row longer than a wave of 16-byte lanes": (((1, 2, 3, 272), (2, 2, 100), (1, 1, 90)), 1, 5, 4),
    "row longer than a wave of dword lanes": (((1, 2, 3, 70), (2, 2, 33), (1, 1, 20)), 0, 4, 1),
    "more sample-channel pairs than one grid dimension holds": (((2, 1, 2, 4), 1, 1), 3, 33000, 4),
}


@pytest.mark.parametrize("name", sorted(_OCCLUDE_CASES))
def test_occlude_windows_is_the_restatement_bit_for_bit(name):
    (shape, win, stride), first, count, lead = _OCCLUDE_CASES[name]
    x = _input(shape, 3)
    fill = np.array([-7.5, 0.1][:shape[0]], dtype=np.float32)
    got = _occlude(x, fill, win, stride, first, count, lead)
    want = O.occlude(x, fill, win, stride, first, count).view(np.uint32)
    assert np.array_equal(got, want)
    wn = O.grid(shape[1:], win, stride)[2]
    if first + count > wn:                                                               # the padding rule: repeats of the last window
        assert all(np.array_equal(got[b], got[wn - 1 - first]) for b in range(wn - first, count))
    if "single window" not in name:                                                      # (there every voxel is the fill)
        assert np.isnan(got.view(np.float32)).any() and (got == 0x80000000).any()        # the planted patterns came through somewhere


# ---- mmnn_occlusion_map -------------------------------------------------------------------------------------------------------------------
def _map(shape3, win, stride, base, scores):
    M, L = _lib()
    k = len(base)
    db, ds = torch.from_numpy(base).to(DEV), torch.from_numpy(scores).to(DEV)
    out = torch.full((k,) + tuple(shape3), float("nan"), device=DEV)
    M.check(L.mmnn_occlusion_map(ctypes.byref(_desc((1,) + tuple(shape3), win, stride)), k, db.data_ptr(), ds.data_ptr(), out.data_ptr(),
                                 _stream()), "mmnn_occlusion_map")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["A", "B"])
def test_occlusion_map_equals_the_restatement(grid, k):
    shape, win, stride = grid
    rng = np.random.default_rng(10 + k)
    wn = O.grid(shape[1:], win, stride)[2]
    base, scores = rng.standard_normal(k).astype(np.float32), rng.standard_normal((wn, k)).astype(np.float32)
    got = _map(shape[1:], win, stride, base, scores)
    assert np.array_equal(got, O.occlusion_map(base, scores, shape[1:], win, stride))
    assert np.array_equal(got.view(np.uint32), _map(shape[1:], win, stride, base, scores).view(np.uint32))      # two calls, bit for bit


@pytest.mark.parametrize("k", [3, 4])
def test_occlusion_map_with_scores_in_lds_and_in_global_memory(k):
    """16^3 voxels with window 1: 4096 windows.  k = 3 fills the LDS stage to its last float, k = 4 reads the scores from global memory."""
    shape, rng = (16, 16, 16), np.random.default_rng(k)
    base, scores = rng.standard_normal(k).astype(np.float32), rng.standard_normal((4096, k)).astype(np.float32)
    got = _map(shape, 1, 1, base, scores)
    assert np.array_equal(got, O.occlusion_map(base, scores, shape, 1, 1))
    assert np.array_equal(got, (base.astype(np.float64)[None] - scores.astype(np.float64)).astype(np.float32).T.reshape(k, 16, 16, 16))


@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=["A", "B"])
def test_voxels_whose_windows_miss_a_planted_cube_are_exactly_zero(grid):
    shape, win, stride = grid
    cube = (slice(1, 3), slice(4, 6), slice(2, 5))
    wn = O.grid(shape[1:], win, stride)[2]
    hit = O.windows_meeting(cube, shape[1:], win, stride)
    assert 0 < len(hit) < wn
    rng = np.random.default_rng(21)
    base = rng.standard_normal(2).astype(np.float32)
    scores = np.tile(base, (wn, 1))
    scores[hit] += (0.5 + rng.random((len(hit), 2))).astype(np.float32)
    got = _map(shape[1:], win, stride, base, scores)
    assert np.array_equal(got, O.occlusion_map(base, scores, shape[1:], win, stride))
    cover = [O.axis_cover(L, w, s) for L, w, s in zip(shape[1:], win, stride)]
    _, n, _ = O.grid(shape[1:], win, stride)
    untouched = np.ones(shape[1:], dtype=bool)
    for z in range(shape[1]):
        for y in range(shape[2]):
            for x in range(shape[3]):
                untouched[z, y, x] = not any((a * n[1] + b) * n[2] + c in hit for a in cover[0][z] for b in cover[1][y] for c in cover[2][x])
    assert untouched.any() and not untouched.all()
    assert (got[:, untouched] == 0.0).all() and (got[:, ~untouched] < 0.0).all()         # hiding the cube RAISED the scores: negative


# ---- mmnn_channel_means ---------------------------------------------------------------------------------------------------------------------
def _means(x, lead=0):
    M, L = _lib()
    c, n = x.shape
    buf = torch.zeros(lead + x.size, device=DEV)
    buf[lead:].copy_(torch.from_numpy(x).reshape(-1))
    out = torch.full((c,), float("nan"), device=DEV)
    ws = torch.empty(c * M.CHANNEL_MEANS_PARTS, dtype=torch.float64, device=DEV)
    M.check(L.mmnn_channel_means(buf.data_ptr() + 4 * lead, c, n, out.data_ptr(), ws.data_ptr(), _stream()), "mmnn_channel_means")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [9 * 10 * 13, 32 ** 3, 3, 257 * 4 + 2])
def test_channel_means_round_the_fp64_mean(n):
    """Non-negative data: an fp64 sum of n <= 2^24 such fp32 values is off by at most n * 2^-53 relative, far below half an fp32 ulp, so
    the result must be one of the two fp32 neighbours of the fp64 mean."""
    x = np.random.default_rng(n).random((2, n)).astype(np.float32) * np.float32(3.0)
    got = _means(x)
    mean = x.astype(np.float64).mean(axis=1)
    r = mean.astype(np.float32)
    lo = np.where(r.astype(np.float64) > mean, np.nextafter(r, np.float32(-np.inf)), r)
    hi = np.where(r.astype(np.float64) < mean, np.nextafter(r, np.float32(np.inf)), r)
    print(f"n = {n}: got {got!r}, fp64 mean {mean!r}")
    assert got.dtype == np.float32 and ((got == lo) | (got == hi)).all()
    assert np.array_equal(got.view(np.uint32), _means(x).view(np.uint32))                # two calls, bit for bit
    assert np.array_equal(got.view(np.uint32), _means(x, lead=1).view(np.uint32))        # off the 16-byte grid: the same order of additions


# ---- OcclusionSensitivity -------------------------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """Two outputs per sample: the fp64 sum over a hidden cube (all channels) and over channel 0, on the GPU."""

    def forward(self, x):
        cube = x[:, :, 2:6, 5:9, 3:8].double().sum(dim=(1, 2, 3, 4))
        first = x[:, 0].double().sum(dim=(1, 2, 3))
        return torch.stack([cube, first], dim=1).float()


def _eighths(shape, seed):
    """Multiples of 1/8 in [-2, 2): every sum of them is exact in fp64, so a channel's mean does not depend on the order of the additions."""
    return (np.random.default_rng(seed).integers(-16, 16, shape) / 8.0).astype(np.float32)


def _restated_maps(model, x, win, stride, batch, fill, clinical=None):
    """(base outputs, maps): the restatement's batches through `model` in the compositions OcclusionSensitivity uses."""
    image = x[0]
    if fill == "mean":
        fill = (image.astype(np.float64).reshape(image.shape[0], -1).sum(axis=1) / image[0].size).astype(np.float32)
    else:
        fill = np.full(image.shape[0], fill, dtype=np.float32)
    wn = O.grid(image.shape[1:], win, stride)[2]

    def run(batch_np):
        t = torch.from_numpy(batch_np).to(DEV)
        with torch.no_grad():
            if clinical is None:
                return model(t)
            return model({"image": t, "clinical": clinical.expand(t.shape[0], -1).contiguous()})

    base = run(x).cpu().numpy()
    scores = np.empty((wn, base.shape[1]), dtype=np.float32)
    for first in range(0, wn, batch):
        out = run(O.occlude(image, fill, win, stride, first, batch)).cpu().numpy()
        rows = min(batch, wn - first)
        scores[first:first + rows] = out[:rows]
    return base, O.occlusion_map(base[0], scores, image.shape[1:], win, stride)


@pytest.mark.parametrize("fill", [0.75, "mean"])
def test_occlusion_sensitivity_on_a_stub_scorer(fill):
    from mmnn_sts_amd.utils.utils import OcclusionSensitivity
    shape, win, stride = (1, 2, 9, 10, 13), (4, 3, 5), (2, 3, 4)
    x = _eighths(shape, 31)
    model = _Stub().to(DEV)
    occ = OcclusionSensitivity(model, window=win, stride=stride, batch=5, fill=fill)      # 48 windows: a padded last batch
    outputs, maps = occ(torch.from_numpy(x).to(DEV))
    base, want = _restated_maps(model, x, win, stride, 5, fill)
    assert maps.is_cuda and maps.dtype == torch.float32 and tuple(maps.shape) == (2,) + shape[2:]
    assert np.array_equal(outputs.cpu().numpy(), base) and np.array_equal(maps.cpu().numpy(), want)
    got = maps.cpu().numpy()
    assert (got[0][:, :, 12] == 0.0).all() and np.abs(got[0][2:6, 5:9, 3:8]).max() > 0.0  # x = 12 is covered by the window 8..12 only: past the cube
    with pytest.raises(ValueError, match=r"window \(4, 3, 14\) is larger than the input extent \(9, 10, 13\)"):
        OcclusionSensitivity(model, window=(4, 3, 14), stride=1)(torch.from_numpy(x).to(DEV))


def _models():
    from mmnn_sts_amd.models.densenet import TinyDensenet
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    from mmnn_sts_amd.models.resnet import r3d_18
    torch.manual_seed(7)
    return {
        "tinydensenet": lambda: (TinyDensenet(spatial_dims=3, in_channels=1, out_channels=2, feature_channels=12, dropout_prob=0.2), 1, False),
        "fusion": lambda: (MultiModalModel(TinyDensenet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.2),
                                           [f"p{i}" for i in range(32)], 2, 12, blend=False), 2, True),
        "r3d_18": lambda: (r3d_18(2), 1, False),
    }


@pytest.mark.parametrize("name", ["tinydensenet", "fusion", "r3d_18"])
def test_occlusion_sensitivity_on_the_real_models(name):
    """Window 16, stride 8, batch 4 at 32^3: 27 windows, seven batches, the last padded with one repeat."""
    from mmnn_sts_amd.utils.utils import OcclusionSensitivity
    model, channels, multimodal = _models()[name]()
    model = model.to(DEV).eval()
    x = _eighths((1, channels, 32, 32, 32), 41)
    clinical = torch.from_numpy(np.random.default_rng(42).standard_normal((1, 32)).astype(np.float32)).to(DEV) if multimodal else None
    dx = torch.from_numpy(x).to(DEV)
    occ = OcclusionSensitivity(model, window=16, stride=8, batch=4, multimodal=multimodal)
    arg = {"image": dx, "clinical": clinical} if multimodal else dx
    model.train()                                                                        # the wrapper runs the eval forward and restores the mode
    outputs, maps = occ(arg)
    assert model.training and all(m.training for m in model.modules())
    model.eval()
    base, want = _restated_maps(model, x, 16, 8, 4, "mean", clinical)
    got = maps.cpu().numpy()
    assert tuple(maps.shape) == (base.shape[1], 32, 32, 32) and np.isfinite(got).all() and np.abs(got).max() > 0.0
    assert tuple(occ.scores.shape) == (27, base.shape[1])
    assert np.array_equal(outputs.cpu().numpy(), base)
    assert np.array_equal(got, want)
    again_outputs, again = occ(arg)
    assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32)) and torch.equal(again_outputs, outputs)


# ---- the CLI, one fresh process each ---------------------------------------------------------------------------------------------------------
_run = functools.partial(run_main, limit_s=300)


@pytest.mark.parametrize("gradcam", [True, False], ids=["gradcam on", "no_gradcam"])
def test_cli_writes_one_map_per_synthetic_patient(tmp_path, gradcam):
    log = _run(["--inference", "--images", "--survival", "--occlusion", "--synthetic_size", "32", "--synthetic_patients", "4",
                "--config", tiny_config(tmp_path, "t1", 1)] + ([] if gradcam else ["--no_gradcam"]), tmp_path)
    assert "All C-indexes" in log
    written = sorted(p.name for p in (tmp_path / "attention_maps").iterdir())
    patients = 2                                                                         # max(2, synthetic_patients // 4)
    assert written == sorted([f"patient{i}_occ_map.npy" for i in range(patients)] +
                             ([f"patient{i}_att_map.npy" for i in range(patients)] if gradcam else []))
    for i in range(patients):
        m = np.load(tmp_path / "attention_maps" / f"patient{i}_occ_map.npy")
        assert m.shape == (2, 32, 32, 32) and m.dtype == np.float32 and np.isfinite(m).all() and np.abs(m).max() > 0.0


def test_cli_writes_the_maps_on_every_scan(tmp_path):
    from mmnn_sts_amd.data import ingest, nifti, synth_nifti
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    from mmnn_sts_amd.models.densenet import TinyDensenet
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    from tests import _resample_ref as G
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=4, seed=43, val_fraction=0.5)
    for i, uid in enumerate(tree["uids"]):                                               # a geometry of its own for every scan
        for k, mod in enumerate(("t1", "t2")):
            path = os.path.join(tree["image_loc"], mod, f"SYN-{i:04d}-{mod}-a", f"scan_{mod}.nii.gz")
            img = nifti.read(path)
            A = G.affine((("z", 0.04 + 0.01 * i), ("x", -0.02 * (k + 1))), (0.9, 0.8 + 0.1 * k, 3.0), (-40.5 + i, 22.25, -13.0 * (k + 1)))
            nifti.write(path, img.raw, img.slope, img.inter, affine=A)
    torch.manual_seed(5)
    img_model = TinyDensenet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.2)
    weights = tmp_path / "fresh.pth"
    torch.save(MultiModalModel(img_model, [f"predictor{i}" for i in range(32)], 2, 12, blend=False).state_dict(), weights)
    _run(["--inference", "--images", "--preop", "--survival", "--transforms", "--scan_space", "--occlusion", "--weights", str(weights),
          "--config", tiny_config(tmp_path), "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
          "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]], tmp_path)
    val_uids = [int(l) for l in open(tree["val_uids"]).read().split()]
    assert len(val_uids) == 2
    ds = T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])
    collate = ingest.IngestCollate(DEV, keep_workspaces=True)
    for i, uid in enumerate(val_uids):
        d = tmp_path / "attention_maps" / f"_patient_{uid}"
        occ = np.load(tmp_path / "attention_maps" / f"patient{i}_occ_map.npy")
        assert occ.shape == (2, 64, 64, 64) and occ.dtype == np.float32 and np.isfinite(occ).all() and np.abs(occ).max() > 0.0
        # today's files keep their names; the occlusion maps sit beside them
        assert sorted(p.name for p in d.iterdir()) == sorted(
            ["t1image.nii.gz", "t2image.nii.gz", "att_map.nii.gz", "preds.txt"] + [f"occ_map_class{k}.nii.gz" for k in range(2)] +
            [f"{prefix}_class{k}_on_{m}.nii.gz" for prefix in ("att_map", "occ_map") for k in range(2) for m in ("t1", "t2")])
        assert (tmp_path / "attention_maps" / f"patient{i}_att_map.npy").exists()
        for k in range(2):
            assert np.array_equal(nifti.read(str(d / f"occ_map_class{k}.nii.gz")).raw, occ[k])
        item = ds.getDataByUID(uid)
        collate([item])
        for (scan, _), kept, mod in zip(item[0].volumes, collate.last_volumes[0], ("t1", "t2")):
            want = ingest.maps_to_scan(torch.from_numpy(occ).to(DEV), kept.shape, kept.workspace).cpu().numpy()       # (k, z, y, x)
            for k in range(2):
                got = nifti.read(str(d / f"occ_map_class{k}_on_{mod}.nii.gz"))
                assert got.raw.dtype == np.float32 and got.raw.shape == tuple(scan.shape) and np.array_equal(got.affine, scan.affine)
                assert not np.array_equal(got.affine, np.eye(4))
                assert np.array_equal(got.raw, want[k].transpose(2, 1, 0))
