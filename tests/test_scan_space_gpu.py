"""The inverse path of the ingest (`mmnn_maps_to_scan`, csrc/ingest.hip; `ingest.maps_to_scan`) against the fp64 restatement of its
contract in tests/_scan_space_ref.py: a scan is ingested, then 64^3 maps are laid back over its grid from the ingest's own workspace.

Bound: the extents equal the restatement's EXACTLY; a voxel is zero on the device exactly where the restatement's is (the maps are drawn
from [0.25, 1], so every kept voxel is a convex combination of values >= 0.25 and every dropped one is 0); elsewhere the two agree within
2 * 2^-24 * max|map| absolute.  Derivation: the device forms the blend in fp64 like the restatement, so its one visible error is the
final rounding to fp32 of a value of magnitude at most max|map| -- half a unit; the order of the fp64 operations adds ~1e-16 relative; two
units are allowed, the convention of `_ingest_ref.tolerance`."""
import numpy as np
import pytest
import torch

from mmnn_sts_amd.data import ingest
from tests import _ingest_ref as R
from tests import _resample_ref as G
from tests import _scan_space_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
SENTINEL = 1.0e30          # no output can hold it: the maps are at most 1


def _holey_mask(shape):
    """A box well inside the volume with interior empty slices on all three axes."""
    lo = tuple(max(1, n // 8) for n in shape)
    hi = tuple(n - max(2, n // 6) for n in shape)
    holes = tuple((lo[a] + 2, lo[a] + 3, hi[a] - 3) for a in range(3))
    return R.box_mask(shape, lo, hi, holes)


def _maps(rng, n):
    return (0.25 + 0.75 * rng.random((n, 64, 64, 64))).astype(np.float32)


def _ingest(scan, mask, ss=(1.0, 0.0), ms=(1.0, 0.0), index_map=None):
    """(the ingest's workspace, its extents)."""
    plane = torch.empty((64, 64, 64), device=DEV)
    ws = torch.empty(ingest.workspace_bytes(*scan.shape), dtype=torch.uint8, device=DEV)
    ext = ingest.ingest_volume(ingest.upload(scan, DEV, *ss), ingest.upload(mask, DEV, *ms), plane, workspace=ws, index_map=index_map)
    return ws, tuple(ext.cpu().tolist())


def _to_scan(maps, shape, ws, lead=None):
    """The device result as an (n, x, y, z) array.  With `lead` the output sits `lead` floats into a larger buffer whose other floats must
    keep their value."""
    n, v = maps.shape[0], int(np.prod(shape))
    dmaps = torch.from_numpy(maps).to(DEV)
    if lead is None:
        out = ingest.maps_to_scan(dmaps, shape, ws)
    else:
        buf = torch.full((lead + n * v + GUARD,), SENTINEL, device=DEV)
        out = ingest.maps_to_scan(dmaps, shape, ws, out=buf[lead:lead + n * v].view(n, *shape[::-1]))
        assert out.data_ptr() == buf.data_ptr() + 4 * lead
        b = buf.cpu().numpy()
        assert (b[:lead] == SENTINEL).all() and (b[lead + n * v:] == SENTINEL).all(), "floats outside `out` were written"
    torch.cuda.synchronize()
    assert tuple(out.shape) == (n, *shape[::-1]) and out.dtype == torch.float32
    return out.cpu().numpy().transpose(0, 3, 2, 1)


def _compare(got, maps, keep, label):
    ref = S.maps_to_scan_ref(maps, keep)
    tol = S.tolerance(maps)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    zeros_differ = int(((got == 0) != (ref == 0)).sum())
    print(f"{label}: kept {tuple(int(k.sum()) for k in keep)} of {got.shape[1:]}, max error {err:.3e}, bound {tol:.3e} ({err / tol:.2f} of it), "
          f"{zeros_differ} voxels zero on one side only")
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert zeros_differ == 0
    assert err <= tol
    return ref


def _check(scan, mask, n_maps=1, ss=(1.0, 0.0), ms=(1.0, 0.0), seed=0, lead=None, label=""):
    _, ext_ref, v = R.ingest_ref(scan, mask, ss, ms)
    keep = S.keep_flags_of(v)
    ws, ext = _ingest(scan, mask, ss, ms)
    assert ext == ext_ref
    if min(ext) > 0:
        assert ext == tuple(int(k.sum()) for k in keep)
    maps = _maps(np.random.default_rng(seed), n_maps)
    got = _to_scan(maps, scan.shape, ws, lead)
    _compare(got, maps, keep, label)
    return got, maps, ext, ws


def test_odd_extents_holes_on_every_axis_scalar_stores():
    shape = (37, 29, 11)
    _, _, ext, _ = _check(R.random_scan(np.random.default_rng(1), shape, 4), _holey_mask(shape), seed=11, label="37x29x11 int16, holey box")
    assert max(ext) < 64 and shape[0] % 4 != 0


def test_shrunk_axis_and_16_byte_stores():
    shape = (152, 70, 9)
    scan = R.random_scan(np.random.default_rng(2), shape, 16)
    _, _, ext, _ = _check(scan, _holey_mask(shape), ss=(0.5, 1000.25), seed=12, label="152x70x9 float32 scaled, holey box")
    assert ext[0] > 64 and shape[0] % 4 == 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_kept_slice_on_an_axis(axis):
    shape = (40, 36, 20)
    lo, hi = [5, 4, 3], [33, 30, 17]
    hi[axis] = lo[axis] + 1
    _, _, ext, _ = _check(R.random_scan(np.random.default_rng(3), shape, 4), R.box_mask(shape, lo, hi), seed=13 + axis, label=f"one slice kept on axis {axis}")
    assert ext[axis] == 1


def test_64_cubed_full_mask_returns_the_map_bit_for_bit():
    shape = (64, 64, 64)
    got, maps, ext, _ = _check(R.random_scan(np.random.default_rng(4), shape, 2), np.ones(shape, dtype=np.uint8), n_maps=2, seed=14, label="64^3, full mask")
    assert ext == shape
    assert np.array_equal(got, maps)                                 # every coordinate an integer, every weight 0


def test_empty_mask_gives_zeros():
    shape = (37, 29, 11)
    got, _, ext, _ = _check(R.random_scan(np.random.default_rng(5), shape, 4), np.zeros(shape, dtype=np.uint8), n_maps=2, seed=15, lead=GUARD, label="empty mask")
    assert ext == (0, 0, 0) and not got.any()


@pytest.mark.parametrize("shape,lead", [((40, 36, 20), GUARD), ((40, 36, 20), GUARD + 1), ((37, 29, 11), GUARD + 3)])
def test_three_maps_land_in_out_only(shape, lead):
    """x % 4 == 0 on a 16-byte boundary (16-byte stores), the same off it and an odd x (single floats)."""
    got, maps, _, _ = _check(R.random_scan(np.random.default_rng(6), shape, 4), _holey_mask(shape), n_maps=3, seed=16, lead=lead, label=f"3 maps, {shape}, lead {lead}")
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


def test_sixteen_maps_and_two_calls_bit_identical():
    shape = (44, 21, 13)
    scan, mask = R.random_scan(np.random.default_rng(7), shape, 4), _holey_mask(shape)
    got, maps, _, ws = _check(scan, mask, n_maps=16, seed=17, label="16 maps")
    again = _to_scan(maps, shape, ws)
    assert np.array_equal(got, again)
    one = _to_scan(maps[5:6], shape, ws)
    assert np.array_equal(one[0], got[5])                            # a map's result does not depend on its neighbours
    with pytest.raises(ValueError):
        ingest.maps_to_scan(torch.zeros((17, 64, 64, 64), device=DEV), shape, ws)
    with pytest.raises(ValueError):
        ingest.maps_to_scan(torch.zeros((1, 64, 64, 64), device=DEV), shape, ws[:64])          # not an ingest workspace of this scan
    with pytest.raises(ValueError):
        ingest.maps_to_scan(torch.zeros((1, 64, 64, 64), device=DEV), shape, ws, out=torch.empty((1, *shape), device=DEV))      # (x, y, z), not (z, y, x)


def test_mask_on_its_own_grid_follows_the_resampled_mask():
    scan_shape, mask_shape, _, _, T = G.case("E")
    scan = R.random_scan(np.random.default_rng(8), scan_shape, 4)
    mask = G.ellipsoid(mask_shape, 40)
    restated, m, c = G.resample_ref(mask, scan_shape, T)
    G.assert_comparable(restated, m, c, mask_shape, 0.5, "case E")
    keep = S.keep_flags(scan, restated)
    ws, ext = _ingest(scan, mask, index_map=T)
    assert ext == tuple(int(k.sum()) for k in keep) and 0 < min(ext) and any(e < n for e, n in zip(ext, scan_shape))
    maps = _maps(np.random.default_rng(18), 2)
    _compare(_to_scan(maps, scan_shape, ws), maps, keep, "case E, mask resampled from its own grid")


def test_collate_keeps_the_workspaces_of_the_last_batch(tmp_path):
    import os
    from mmnn_sts_amd.data import synth_nifti
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    tree = synth_nifti.write_tree(tmp_path, n_patients=2, seed=23)
    ds = T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])
    off = ingest.IngestCollate(DEV)
    x0, _, _ = off([ds[0], ds[1]])
    assert off.last_volumes == []
    on = ingest.IngestCollate(DEV, keep_workspaces=True)
    x1, _, _ = on([ds[0], ds[1]])
    assert torch.equal(x0, x1)                                       # the batch does not depend on whose workspace was used
    assert len(on.last_volumes) == 2 and all(len(p) == 2 for p in on.last_volumes)
    maps = _maps(np.random.default_rng(19), 2)
    for n in range(2):
        for c, (scan, mask) in enumerate(ds[n][0].volumes):
            kv = on.last_volumes[n][c]
            assert kv.shape == scan.shape and np.array_equal(kv.affine, scan.affine)
            keep = S.keep_flags(scan.raw, mask.raw, (scan.slope, scan.inter), (mask.slope, mask.inter))
            _compare(_to_scan(maps, kv.shape, kv.workspace), maps, keep, f"patient {n}, channel {c}")


def test_512x512x48_once():
    shape = (512, 512, 48)
    scan = np.random.default_rng(9).integers(1, 3000, shape, dtype=np.int16)
    mask = R.box_mask(shape, (96, 101, 4), (416, 411, 43), holes=((200,), (300, 301), (20,)))
    _, _, ext, _ = _check(scan, mask, n_maps=2, ss=(0.25, -12.5), seed=20, label="512x512x48 int16, 320x310x39 box with holes")
    assert ext == (319, 308, 38)
