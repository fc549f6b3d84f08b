"""The scan ingest, the way back and the transform pipelines at a chosen volume size S (1..128) against the fp64 restatements of
tests/_ingest_sized_ref.py and tests/test_transforms_gpu.py, and `main.py --image_size 128` as fresh processes on a synthetic NIfTI tree.

Bounds, none of which depends on S (tests/_ingest_ref.py, tests/_scan_space_ref.py): the extents are equal EXACTLY; the plane is within
2 * 2^-24 * max|v| absolute; the way back is zero exactly where the restatement is and within 2 * 2^-24 * max|map| elsewhere.  The
transform pipelines keep the tolerances tests/test_transforms_gpu.py holds the same stages to.

The sizes: 24 -- lanes beyond S idle, 64 -- the default, 100 -- neither a multiple of 64 nor of the waves per block, so the last block of
pass C has waves without a z window, 128 -- two windows per lane, the cap.  The (97, 130, 23) scan keeps (66, 90, 15): below and above S at
24 and 64, all below S at 100 and 128 (replication on every axis); kept extents above 128 come from the (150, 140, 40) scan, (149, 88, 39).

The `ingest_ws` of `maps_to_scan` holds the scan's kept slices and nothing of the S its ingest wrote a plane at, so the maps' S is their
own: it need not equal the ingest's, and the call has nothing to check it against (`test_maps_size_need_not_be_the_ingests`)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd import transforms as T
from mmnn_sts_amd.data import ingest, synth_nifti
from tests import _ingest_ref as R
from tests import _ingest_sized_ref as Z
from tests import _scan_space_ref as S
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (97, 130, 23)
GUARD = 256
SENTINEL = 1.0e30          # no plane or map output can hold it
_cache = {}


def _holey_mask(shape):
    """A box well inside the volume with interior empty slices on all three axes (as tests/test_ingest_gpu.py draws it)."""
    lo = tuple(max(1, n // 8) for n in shape)
    hi = tuple(n - max(2, n // 6) for n in shape)
    holes = tuple((lo[a] + 2, lo[a] + 3, hi[a] - 3) for a in range(3))
    return R.box_mask(shape, lo, hi, holes)


def _case(name):
    """(scan, mask) of a named case, built once."""
    if name not in _cache:
        if name == "holey":
            _cache[name] = (R.random_scan(np.random.default_rng(104), SHAPE, 4), _holey_mask(SHAPE))
        elif name == "faces":
            shape = (150, 140, 40)
            _cache[name] = (R.random_scan(np.random.default_rng(8), shape, 16),
                            R.box_mask(shape, (0, 0, 0), (150, 90, 40), holes=((70,), (40, 41), (17,))))      # the box touches five faces
        elif name == "empty":
            _cache[name] = (_case("holey")[0], np.zeros(SHAPE, dtype=np.uint8))
        else:
            shape = {"odd": (37, 29, 11), "sixteen": (44, 21, 13)}[name]
            _cache[name] = (R.random_scan(np.random.default_rng(sum(shape)), shape, 4), _holey_mask(shape))
    return _cache[name]


def _uploaded(name, ss=(1.0, 0.0)):
    key = ("dev", name, ss)
    if key not in _cache:
        scan, mask = _case(name)
        _cache[key] = (ingest.upload(scan, DEV, *ss), ingest.upload(mask, DEV))
    return _cache[key]


def _plane_ref(name, size, ss=(1.0, 0.0)):
    key = ("ref", name, size, ss)
    if key not in _cache:
        _cache[key] = Z.ingest_ref(*_case(name), size, ss)
    return _cache[key]


def _check_plane(name, size, ss=(1.0, 0.0)):
    ref, ext_ref, v = _plane_ref(name, size, ss)
    s, m = _uploaded(name, ss)
    out = torch.full((size,) * 3, float("nan"), device=DEV)
    ext = tuple(ingest.ingest_volume(s, m, out).cpu().tolist())
    got = out.cpu().numpy()
    tol = R.tolerance(v)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{name} at S = {size}: extents {ext} (ref {ext_ref}), max error {err:.3e}, bound {tol:.3e} ({err / tol if tol else 0.0:.2f} of it), "
          f"NaN {int(np.isnan(got).sum())}")
    assert ext == ext_ref
    assert not np.isnan(got).any()                                   # every one of the S^3 floats was written
    assert err <= tol
    return out, ext


# ---- the ingest --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [24, 64, 100, 128])
def test_ingest_parity_at_size(size):
    _, ext = _check_plane("holey", size, (0.5, 3.0))
    assert ext == (66, 90, 15) and min(ext) < size                   # z is replicated at every S
    if size in (24, 64):
        assert max(ext) > size                                       # ... and x, y are shrunk


def test_ingest_parity_128_box_on_five_faces():
    _, ext = _check_plane("faces", 128)
    assert ext == (149, 88, 39) and ext[0] > 128 > ext[1]


def test_size_64_equals_the_unsized_call_bit_for_bit():
    s, m = _uploaded("holey", (0.5, 3.0))
    sized, ext = _check_plane("holey", 64, (0.5, 3.0))
    plain = torch.full((64, 64, 64), float("nan"), device=DEV)
    ext_plain = torch.empty(3, dtype=torch.int32, device=DEV)
    ws = torch.empty(ingest.workspace_bytes(*SHAPE), dtype=torch.uint8, device=DEV)
    desc = _lib.IngestDesc(*SHAPE, s.datatype, m.datatype, s.slope, s.inter, m.slope, m.inter)
    with torch.cuda.device(torch.device(DEV)):
        _lib.check(_lib.lib().mmnn_ingest_volume(ctypes.byref(desc), s.data.data_ptr(), m.data.data_ptr(), plain.data_ptr(), ext_plain.data_ptr(),
                                                 ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "mmnn_ingest_volume")
    torch.cuda.synchronize()
    assert tuple(ext_plain.cpu().tolist()) == ext
    assert torch.equal(plain.cpu(), sized.cpu())


def test_empty_mask_at_100_writes_every_zero():
    out, ext = _check_plane("empty", 100, (2.0, 1.0))
    assert ext == (0, 0, 0) and out.shape == (100, 100, 100) and not out.cpu().numpy().any()


def test_plane_at_100_lands_in_its_channel_only():
    s, m = _uploaded("holey", (0.5, 3.0))
    batch = torch.full((2, 2, 100, 100, 100), SENTINEL, device=DEV)
    ingest.ingest_volume(s, m, batch[1, 0])
    torch.cuda.synchronize()
    b = batch.cpu()
    assert (b[0] == SENTINEL).all() and (b[1, 1] == SENTINEL).all() and not (b[1, 0] == SENTINEL).any()
    ref, _, v = _plane_ref("holey", 100, (0.5, 3.0))
    assert np.abs(b[1, 0].double().numpy() - ref).max() <= R.tolerance(v)


@pytest.mark.parametrize("size", [100, 128])
def test_two_ingests_are_bit_identical(size):
    s, m = _uploaded("holey", (0.5, 3.0))
    a, b = torch.empty((size,) * 3, device=DEV), torch.full((size,) * 3, SENTINEL, device=DEV)
    ingest.ingest_volume(s, m, a)
    ingest.ingest_volume(s, m, b)
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), b.cpu())


# ---- the way back --------------------------------------------------------------------------------------------------------------------
def _workspace(name, size):
    """(the workspace an ingest of the case at S = size left, the keep flags of the restatement)."""
    key = ("ws", name, size)
    if key not in _cache:
        scan, mask = _case(name)
        s, m = _uploaded(name)
        ws = torch.empty(ingest.workspace_bytes(*scan.shape), dtype=torch.uint8, device=DEV)
        ext = ingest.ingest_volume(s, m, torch.empty((size,) * 3, device=DEV), workspace=ws)
        keep = S.keep_flags(scan, mask)
        assert tuple(ext.cpu().tolist()) == tuple(int(k.sum()) for k in keep)
        _cache[key] = (ws, keep)
    return _cache[key]


def _to_scan(maps, shape, ws, lead):
    """The device result as an (n, x, y, z) array; the output sits `lead` floats into a larger buffer whose other floats must keep their value."""
    n, v = maps.shape[0], int(np.prod(shape))
    buf = torch.full((lead + n * v + GUARD,), SENTINEL, device=DEV)
    out = ingest.maps_to_scan(torch.from_numpy(maps).to(DEV), shape, ws, out=buf[lead:lead + n * v].view(n, *shape[::-1]))
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:lead] == SENTINEL).all() and (b[lead + n * v:] == SENTINEL).all(), "floats outside `out` were written"
    return out.cpu().numpy().transpose(0, 3, 2, 1)


def _compare(got, maps, keep, label):
    ref = Z.maps_to_scan_ref(maps, keep)
    tol = S.tolerance(maps)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    zeros_differ = int(((got == 0) != (ref == 0)).sum())
    print(f"{label}: kept {tuple(int(k.sum()) for k in keep)} of {got.shape[1:]}, max error {err:.3e}, bound {tol:.3e} ({err / tol:.2f} of it), "
          f"{zeros_differ} voxels zero on one side only")
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert zeros_differ == 0
    assert err <= tol


def _maps(seed, n, size):
    return (0.25 + 0.75 * np.random.default_rng(seed).random((n, size, size, size))).astype(np.float32)


@pytest.mark.parametrize("size", [24, 100, 128])
def test_three_maps_back_onto_an_odd_grid(size):
    shape = _case("odd")[0].shape
    ws, keep = _workspace("odd", size)
    maps = _maps(size, 3, size)
    got = _to_scan(maps, shape, ws, GUARD + 3)                       # odd x, off every 16-byte boundary: single floats
    _compare(got, maps, keep, f"3 maps of {size}^3 on {shape}")
    assert shape[0] % 4 != 0 and not np.array_equal(got[0], got[1])


def test_sixteen_maps_of_128_fill_the_lds_and_do_not_depend_on_their_neighbours():
    shape = _case("sixteen")[0].shape
    ws, keep = _workspace("sixteen", 128)
    maps = _maps(17, 16, 128)
    got = _to_scan(maps, shape, ws, GUARD)                           # x % 4 == 0 on a 16-byte boundary: 16-byte stores
    _compare(got, maps, keep, f"16 maps of 128^3 on {shape}")
    assert np.array_equal(got, _to_scan(maps, shape, ws, GUARD))     # two calls are bit-identical
    one = _to_scan(maps[5:6], shape, ws, GUARD)
    assert np.array_equal(one[0], got[5])


def test_maps_size_need_not_be_the_ingests():
    shape = _case("odd")[0].shape
    ws, keep = _workspace("odd", 128)                                # kept slices of an ingest at 128 ...
    for size in (24, 64):                                            # ... lay maps of any other S back: nothing of S is in the workspace
        maps = _maps(size + 1, 1, size)
        _compare(_to_scan(maps, shape, ws, GUARD), maps, keep, f"a {size}^3 map over the workspace of an ingest at 128")


def test_refusals():
    s, m = _uploaded("odd")
    ws, _ = _workspace("odd", 24)
    shape = _case("odd")[0].shape
    with pytest.raises(ValueError, match=r"1\.\.128"):
        ingest.ingest_volume(s, m, torch.empty((129, 129, 129), device=DEV))
    with pytest.raises(ValueError, match=r"1\.\.128"):
        ingest.ingest_volume(s, m, torch.empty((100, 100, 64), device=DEV))
    with pytest.raises(ValueError, match=r"1\.\.128"):
        ingest.maps_to_scan(torch.zeros((1, 64, 64, 100), device=DEV), shape, ws)
    with pytest.raises(ValueError, match=r"1\.\.128"):
        ingest.maps_to_scan(torch.zeros((1, 129, 129, 129), device=DEV), shape, ws)
    with pytest.raises(ValueError):
        ingest.maps_to_scan(torch.zeros((17, 100, 100, 100), device=DEV), shape, ws)
    with pytest.raises(ValueError):
        ingest.maps_to_scan(torch.zeros((1, 100, 100, 100), device=DEV), shape, ws[:64])       # not an ingest workspace of this scan


def test_collate_at_128_equals_the_single_volume_results(tmp_path):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    tree = synth_nifti.write_tree(tmp_path, n_patients=2, seed=21)
    ds = T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])
    x, _, _ = ingest.IngestCollate(DEV, size=128)([ds[0], ds[1]])
    assert x.shape == (2, 2, 128, 128, 128) and x.dtype == torch.float32 and x.is_cuda
    for n in range(2):
        for c, (scan, mask) in enumerate(ds[n][0].volumes):
            single = torch.empty((128, 128, 128), device=DEV)
            ingest.ingest_volume(scan, mask, single)
            assert torch.equal(single, x[n, c])
    ref, _, v = Z.ingest_ref(ds[0][0].volumes[1][0].raw, ds[0][0].volumes[1][1].raw, 128, (ds[0][0].volumes[1][0].slope, ds[0][0].volumes[1][0].inter))
    assert np.abs(x[0, 1].double().cpu().numpy() - ref).max() <= R.tolerance(v)


# ---- the transform pipelines at 128 -----------------------------------------------------------------------------------------------------
def _check_pipeline(pipe, x, params, tol):
    from tests.test_transforms_gpu import restate
    out = pipe.apply(x.to(DEV), params)
    torch.cuda.synchronize()
    out = out.cpu().double()
    assert out.shape == (x.shape[0], x.shape[1], 128, 128, 128)
    for i, p in enumerate(params):
        ref = restate(x[i], pipe.stages, p, size=(128,) * 3)
        assert out[i].shape == ref.shape
        err = float((out[i] - ref).abs().max())
        print(f"sample {i}: max error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (i, err, tol)


def test_val_pipeline_at_128():
    from tests.test_transforms_gpu import _raw
    val = T.pipelines(128)[1]
    x = _raw((2, 2, 128, 128, 128), 22)
    _check_pipeline(val, x, val.randomize(2), 1e-5)
    small = val(_raw((1, 2, 37, 50, 43), 22).to(DEV))                # and it resizes up to 128^3 like any other Resize
    assert small.shape == (1, 2, 128, 128, 128)


def test_train_pipeline_all_stages_at_128():
    from tests.test_transforms_gpu import _all_params, _raw
    train = T.pipelines(128)[0]
    x = _raw((2, 2, 128, 128, 128), 21)
    params = [_all_params(), _all_params(theta=-3.0, flip_axis=2, zoom=1.08, gamma=0.8, alpha=27.0)]
    _check_pipeline(train, x, params, 4e-5 * (1 + 2 * 27.0))


# ---- main.py --image_size 128, fresh processes, one at a time -------------------------------------------------------------------------------
_main = functools.partial(run_main, limit_s=600)


def test_cli_training_then_scan_space_inference_at_128(tmp_path):
    tree = synth_nifti.write_tree(tmp_path / "tree", n_patients=4, seed=41, val_fraction=0.5)      # (every event of this tree is observed)
    cfg = tiny_config(tmp_path)
    loc = ["--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]
    log = _main(["--images", "--preop", "--survival", "--blend", "--transforms", "--image_size", "128", "--epochs", "1", "--config", cfg, *loc], tmp_path)
    assert "epoch 1/1" in log and os.path.exists(tmp_path / "best_surv_model.pth"), log[-2000:]
    log = _main(["--inference", "--scan_space", "--image_size", "128", "--images", "--preop", "--survival", "--transforms",
                 "--weights", str(tmp_path / "best_surv_model.pth"), "--config", cfg, *loc], tmp_path)
    assert "All C-indexes" in log
    att = np.load(tmp_path / "attention_maps" / "patient0_att_map.npy")
    assert att.shape == (128, 128, 128) and np.isfinite(att).all()
    uid = [int(l) for l in open(tree["val_uids"]).read().split()][0]
    d = tmp_path / "attention_maps" / f"_patient_{uid}"
    for name in ("t1image", "t2image", "att_map"):
        assert R.read_nifti_file(d / f"{name}.nii.gz")["dim"][:4] == (3, 128, 128, 128)
    assert np.array_equal(R.read_nifti_file(d / "att_map.nii.gz")["data"], att)
    for mod in ("t1", "t2"):
        folder = os.path.join(tree["image_loc"], mod, f"SYN-{tree['uids'].index(uid):04d}-{mod}-a")
        scan, mask = R.read_nifti_file(os.path.join(folder, f"scan_{mod}.nii.gz")), R.read_nifti_file(os.path.join(folder, "mask.nii.gz"))
        on = R.read_nifti_file(d / f"att_map_class0_on_{mod}.nii.gz")
        assert on["datatype"] == 16 and on["dim"][:4] == scan["dim"][:4] and on["dim"][0] == 3          # the scan's extents
        keep = S.keep_flags(scan["data"], mask["data"], (scan["scl_slope"], scan["scl_inter"]))
        _compare(on["data"][None], att[None], keep, f"class 0 of patient {uid} on its {mod} scan")
