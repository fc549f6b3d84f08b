"""`mmnn_mask_margin` on the device against the numpy restatement (tests/_mask_margin_ref.py), `out` and `dist2` bit for bit in both modes:
points exactly on the sphere, anisotropic and random spacings, a reach of 0 along z and a reach above the extents, set voxels on every
face and corner, extents that cross a tile boundary along each axis, every mask type code under a scaling, a NaN voxel, `dist2` null,
guard bytes around `out` and `dist2`, two calls, and every refusal of the contract."""
import ctypes

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import ingest
from tests import _mask_margin_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 256, 0xA5
ANISO = (0.8, 0.8, 5.0)


def _device(raw, spacing, radius, mode, slope=1.0, inter=0.0, with_dist2=True):
    """`ingest.mask_margin` into `out` / `dist2` carved out of guarded buffers -> (out (x, y, z) uint8, dist2 (x, y, z) or None)."""
    x, y, z = raw.shape
    n = x * y * z
    vol = ingest.upload(raw, DEV, slope, inter)
    ob = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    db = torch.full((n + 2 * GUARD // 8,), -1.5, dtype=torch.float64, device=DEV) if with_dist2 else None
    res = ingest.mask_margin(vol, spacing, radius, mode, out=ob[GUARD:GUARD + n], dist2=None if db is None else db[GUARD // 8:GUARD // 8 + n])
    assert (res.datatype, res.slope, res.inter, res.shape) == (2, 1.0, 0.0, (x, y, z))
    o = ob.cpu().numpy()
    assert (o[:GUARD] == PATTERN).all() and (o[GUARD + n:] == PATTERN).all(), "bytes outside `out` were written"
    out = o[GUARD:GUARD + n].reshape(z, y, x).transpose(2, 1, 0)
    if db is None:
        return out, None
    d = db.cpu().numpy()
    assert (d[:GUARD // 8] == -1.5).all() and (d[GUARD // 8 + n:] == -1.5).all(), "doubles outside `dist2` were written"
    return out, d[GUARD // 8:GUARD // 8 + n].reshape(z, y, x).transpose(2, 1, 0)


def _check(raw, spacing, radius, slope=1.0, inter=0.0, how="separable", modes=("dilate", "shell")):
    for mode in modes:
        want_out, want_d = M.margin(raw, spacing, radius, mode, slope, inter, how)
        out, d = _device(raw, spacing, radius, mode, slope, inter)
        assert np.array_equal(out, want_out), (mode, int((out != want_out).sum()))
        assert np.array_equal(d.view(np.int64), want_d.view(np.int64)), (mode, int((d != want_d).sum()))
    return want_out


def test_points_exactly_on_the_sphere():
    raw = np.zeros((13, 13, 13), dtype=np.uint8)
    raw[6, 6, 6] = 1
    _check(raw, (1.0, 1.0, 1.0), 5.0, how="brute")
    out, d = _device(raw, (1.0, 1.0, 1.0), 5.0, "dilate")
    for off in [(3, 4, 0), (0, 3, 4), (5, 0, 0), (-3, 0, -4), (0, -5, 0)]:
        p = tuple(6 + v for v in off)
        assert out[p] == 1 and d[p] == 25.0, off
    assert out[10, 10, 6] == 0 and np.isinf(d[10, 10, 6])                 # (4, 4, 0): 32 > 25
    assert out[6, 6, 6] == 1 and d[6, 6, 6] == 0.0
    shell, _ = _device(raw, (1.0, 1.0, 1.0), 5.0, "shell")
    assert shell[6, 6, 6] == 0 and shell[9, 10, 6] == 1 and int(shell.sum()) == int(out.sum()) - 1


@pytest.mark.parametrize("spacing", [ANISO, "random"])
@pytest.mark.parametrize("which", ["one_voxel_in_plane", "nothing_along_z", "7.3", "12", "past_every_extent"])
def test_random_masks(spacing, which):
    """37 x 21 x 9 at 3 %, at (0.8, 0.8, 5) and at a random spacing (ascending, so z is the coarse axis as on a scanner): a radius just
    above the finest spacing, one just below the coarsest (reach 0 along z), two in between and one that reaches past every extent."""
    shape = (37, 21, 9)
    if spacing == "random":
        spacing = tuple(sorted(float(v) for v in np.random.default_rng(11).uniform(0.5, 3.0, 3)))
    radius = {"one_voxel_in_plane": 1.01 * min(spacing), "nothing_along_z": 0.99 * max(spacing), "7.3": 7.3, "12": 12.0,
              "past_every_extent": 1.01 * max(n * s for n, s in zip(shape, spacing))}[which]
    reach = M.reach(spacing, radius)
    print("spacing", spacing, "radius", radius, "reach", reach)
    if which == "nothing_along_z":
        assert reach[2] == 0 and reach[0] >= 1
    if which == "past_every_extent":
        assert all(k >= n for k, n in zip(reach, shape)) and max(reach) <= _lib.MARGIN_MAX_REACH
    _check(M.random_mask(shape, 0.03, 5), spacing, radius, how="brute")


def test_reach_zero_along_z_and_reach_above_every_extent():
    raw = M.random_mask((37, 21, 9), 0.03, 6)
    assert M.reach(ANISO, 4.0) == (5, 5, 0) and all(k > n for k, n in zip(M.reach(ANISO, 60.0), (37, 21, 9)))
    flat = _check(raw, ANISO, 4.0, how="brute")
    assert not flat[:, :, ~raw.any(axis=(0, 1))].any()                    # nothing crosses a slice
    _check(raw, ANISO, 60.0, how="brute")


def test_set_voxels_on_every_face_and_corner():
    shape = (19, 17, 7)
    raw = np.zeros(shape, dtype=np.uint8)
    for c in np.ndindex(2, 2, 2):
        raw[tuple(k * (n - 1) for k, n in zip(c, shape))] = 1
    for axis in range(3):
        for side in (0, shape[axis] - 1):
            p = [n // 2 for n in shape]
            p[axis] = side
            raw[tuple(p)] = 1
    _check(raw, (1.1, 0.7, 2.5), 4.0, how="brute")


@pytest.mark.parametrize("shape", [(300, 5, 3), (3, 130, 2), (5, 3, 70), (259, 3, 2), (34, 67, 3)])
def test_extents_that_cross_a_tile_boundary(shape):
    """256 outputs along x per workgroup of the x pass, 16 columns x 64 outputs per y / z tile; 259 and 34 are no multiple of 4."""
    raw = M.random_mask(shape, 0.02, 9)
    raw[shape[0] - 1, shape[1] - 1, shape[2] - 1] = 1
    _check(raw, (0.7, 0.9, 1.3), 6.5)


def test_reach_at_the_cap():
    """Reach 128 along x and y at extents above it: the widest tile the y pass stages, and the longest walk of the x pass."""
    raw = np.zeros((150, 140, 3), dtype=np.uint8)
    raw[0, 0, 0] = raw[149, 139, 2] = raw[20, 130, 1] = 1
    assert M.reach((1.0, 1.0, 40.0), 128.0) == (128, 128, 3)
    _check(raw, (1.0, 1.0, 40.0), 128.0)


def test_empty_and_full_mask():
    for fill in (0, 1):
        raw = np.full((21, 9, 5), fill, dtype=np.uint8)
        for mode in ("dilate", "shell"):
            out, d = _device(raw, ANISO, 7.0, mode)
            assert (out == (fill if mode == "dilate" else 0)).all()
            assert (d == 0.0).all() if fill else np.isinf(d).all()


@pytest.mark.parametrize("dtype", ["uint8", "int16", "int32", "float32", "float64", "int8", "uint16", "uint32"])
def test_every_mask_type_under_a_scaling_that_sets_a_raw_zero(dtype):
    rng = np.random.default_rng(3)
    raw = np.zeros((23, 11, 6), dtype=dtype)
    raw[rng.random(raw.shape) < 0.05] = 3
    raw[rng.random(raw.shape) < 0.9] += 2                                    # raw 2 -> 2 * 1.5 - 3 = 0: not set; raw 0 -> -3: set
    slope, inter = 1.5, -3.0
    flags = M.set_voxels(raw, slope, inter)
    assert flags[raw == 0].all() and not flags[raw == 2].any() and 0 < flags.sum() < flags.size
    _check(raw, ANISO, 5.0, slope, inter)
    _check(raw, ANISO, 5.0, 0.0, 7.0, modes=("dilate",))                   # a slope of 0: no scaling, the raw value decides


def test_a_nan_voxel_counts_as_set():
    raw = np.zeros((15, 9, 4), dtype=np.float32)
    raw[7, 4, 2] = np.nan
    want = _check(raw, ANISO, 5.0, how="brute", modes=("dilate",))
    assert want[7, 4, 2] == 1 and want[7, 4, 1] == 1 and want.sum() > 2


def test_dist2_null_and_two_calls_bit_identical():
    raw = M.random_mask((70, 33, 11), 0.03, 8)
    first = _device(raw, ANISO, 10.0, "shell")
    again = _device(raw, ANISO, 10.0, "shell")
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.int64), again[1].view(np.int64))
    alone, none = _device(raw, ANISO, 10.0, "shell", with_dist2=False)
    assert none is None and np.array_equal(alone, first[0])


def test_workspace_reuse_and_the_wrappers_refusals():
    raw = M.random_mask((20, 10, 5), 0.05, 2)
    vol = ingest.upload(raw, DEV)
    ws = torch.empty(ingest.mask_margin_workspace_bytes(20, 10, 5), dtype=torch.uint8, device=DEV)
    a = ingest.mask_margin(vol, ANISO, 5.0, workspace=ws).data.clone()
    b = ingest.mask_margin(vol, ANISO, 5.0, workspace=ws).data
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="workspace"):
        ingest.mask_margin(vol, ANISO, 5.0, workspace=ws[:-1])
    with pytest.raises(ValueError, match="out must be"):
        ingest.mask_margin(vol, ANISO, 5.0, out=torch.empty(999, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="overlap"):
        ingest.mask_margin(vol, ANISO, 5.0, out=vol.data)
    with pytest.raises(ValueError, match="smaller than every voxel spacing"):
        ingest.mask_margin(vol, ANISO, 0.7)


def test_every_refusal_of_the_contract_leaves_the_buffers_alone():
    n = 64
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out = torch.full((n,), PATTERN, dtype=torch.uint8, device=DEV)
    dist2 = torch.full((n,), -1.5, dtype=torch.float64, device=DEV)
    ws = torch.full((ingest.mask_margin_workspace_bytes(4, 4, 4),), PATTERN, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib()

    def desc(x=4, y=4, z=4, code=2, spacing=(1.0, 1.0, 1.0), radius=2.0, mode=_lib.MARGIN_DILATE):
        return _lib.MaskMarginDesc(x, y, z, code, 1.0, 0.0, (ctypes.c_double * 3)(*spacing), radius, mode)

    def refused(d, m=mask.data_ptr(), o=out.data_ptr(), w=ws.data_ptr(), what="mask_margin"):
        assert lib.mmnn_mask_margin(None if d is None else ctypes.byref(d), m, o, dist2.data_ptr(), w, stream) == 1
        assert what in _lib.last_error(), _lib.last_error()

    refused(None, what="null descriptor")
    for kw in ({"m": None}, {"o": None}, {"w": None}):
        refused(desc(), what="null", **kw)
    for bad, what in [(dict(x=0), "non-positive"), (dict(y=-1), "non-positive"), (dict(x=2048, y=2048, z=512), "2^31"), (dict(code=3), "datatype code"),
                      (dict(spacing=(0.0, 1.0, 1.0)), "spacing[0]"), (dict(spacing=(1.0, float("inf"), 1.0)), "spacing[1]"),
                      (dict(spacing=(1.0, 1.0, float("nan"))), "spacing[2]"), (dict(radius=0.0), "radius"), (dict(radius=float("nan")), "radius"),
                      (dict(mode=2), "mode"), (dict(radius=_lib.MARGIN_MAX_REACH + 1.0), "reaches more than")]:
        refused(desc(**bad), what=what)
    refused(desc(), o=mask.data_ptr(), what="overlap")
    refused(desc(), o=mask.data_ptr() + n - 1, what="overlap")
    refused(desc(), w=ws.data_ptr() + 8, what="misaligned")
    torch.cuda.synchronize()
    assert (out == PATTERN).all() and (dist2 == -1.5).all() and (ws == PATTERN).all()
    # the same descriptor is taken once nothing is wrong with it
    assert lib.mmnn_mask_margin(ctypes.byref(desc()), mask.data_ptr(), out.data_ptr(), dist2.data_ptr(), ws.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert (out == 0).all() and torch.isinf(dist2).all()
