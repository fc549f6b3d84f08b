"""The RTSTRUCT path on the device.  `mmnn_rasterize_contours` against the numpy fp64 restatement of its contract (tests/_rtstruct_ref.py),
byte for byte and with the output inside a patterned guard buffer; a synth_nifti tree against its synth_dicom twin with RTSTRUCT masks
through `collate_volumes`, byte for byte; and `main.py` on that twin in one fresh process.

Byte-for-byte is a condition, not a tolerance: the kernel and the restatement round every operation of the crossing abscissa alike,
and the polygons are chosen (seeds fixed on the CPU) so that no crossing lies within 1e-6 of a voxel centre and no vertex within 1e-6 of
a row -- ten orders of magnitude above an fp64 rounding at these extents -- which each test asserts before it compares every voxel."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import ingest, nifti, synth_dicom, synth_nifti
from tests import _resample_ref as G
from tests import _rtstruct_ref as C
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
PATTERN = 0xA5
MARGIN = 1e-6


def _fill(arrays, shape, out_lead=0):
    """The kernel's bytes as an (x, y, z) array; `out` sits inside a larger buffer whose other bytes must keep their pattern."""
    n = shape[0] * shape[1] * shape[2]
    lead = GUARD + out_lead
    buf = torch.full((lead + n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    v = ingest.rasterize_contours(arrays, SimpleNamespace(shape=shape, affine=None), DEV, out=buf[lead:lead + n])
    torch.cuda.synchronize()
    assert v.datatype == 2 and (v.slope, v.inter) == (1.0, 0.0) and v.shape == tuple(shape) and v.data.data_ptr() == buf.data_ptr() + lead
    b = buf.cpu().numpy()
    assert (b[:lead] == PATTERN).all() and (b[lead + n:] == PATTERN).all(), "bytes outside `out` were written"
    return b[lead:lead + n].reshape(shape, order="F")


def _check(per_slice, shape, out_lead=0, exact=False):
    arrays = C.arrays(per_slice, shape[2])
    want, near_x, near_row = C.fill_ref(*arrays, shape)
    print(f"{shape}: {len(arrays[1])} contours, {len(arrays[0])} points, {int(want.sum())} voxels set; smallest |xc - i| {near_x:.3e}, "
          f"smallest vertex-to-row distance {near_row:.3e}")
    if not exact:
        assert near_x >= MARGIN and near_row >= MARGIN, "the case was to keep its crossings and vertices away from the lattice"
    got = _fill(arrays, shape, out_lead)
    assert set(np.unique(got)) <= {0, 1}
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{shape}: {bad.shape[0]} voxels differ, the first at {tuple(bad[0])}: device {got[tuple(bad[0])]}, restatement {want[tuple(bad[0])]}"
    return arrays, want


def _outside(shape, arrays):
    """Whether the points leave the grid's voxel centres on all four sides."""
    p = arrays[0]
    return p[:, 0].min() < 0 and p[:, 1].min() < 0 and p[:, 0].max() > shape[0] - 1 and p[:, 1].max() > shape[1] - 1


def _wide_band(x, k):
    """A wavy band over the whole of a long row and beyond both ends, and two triangles over it near the end of the row."""
    rng = np.random.default_rng([5, k])
    xs = np.sort(rng.uniform(-5.0, x + 5.0, 40))
    upper = np.stack([xs, 2.31 + 0.4 * np.sin(0.013 * xs + k)], axis=1)
    lower = np.stack([xs[::-1], 0.43 + 0.3 * np.cos(0.017 * xs[::-1] + k)], axis=1)
    return [np.concatenate([upper, lower], axis=0), np.array([[1001.3, -1.2], [1012.7, -0.9], [1007.1, 3.5]]),
            np.array([[x - 9.4, 3.3], [x + 3.2, 2.9], [x - 2.7, -2.2]])]


def test_one_voxel():
    hit = np.array([[-0.7, -0.6], [0.8, -0.5], [0.1, 0.9]])
    miss = np.array([[2.3, 1.2], [3.1, 1.4], [2.5, 2.2]])
    assert _check({0: [hit, miss]}, (1, 1, 1))[1].tolist() == [[[1]]]
    assert _check({0: [miss]}, (1, 1, 1))[1].tolist() == [[[0]]]
    assert _check({0: [hit, hit[::-1] * 1.1]}, (1, 1, 1))[1].tolist() == [[[0]]]              # enclosed twice: even


def test_small_and_odd_extents():
    _check(C.stars((5, 3, 2), 0, n=7), (5, 3, 2))
    for seed in (0, 1, 2):
        arrays, want = _check(C.stars((37, 29, 6), seed), (37, 29, 6))
        # the inner star is a hole: the voxel next to the shared centre is outside, one between the two stars inside
        assert 0 < want.sum() < want.size and all(want[18, 14, k] == 0 for k in range(6)) and want[:, :, 0].any()


def test_contours_that_leave_the_grid_an_empty_slice_and_a_contour_outside():
    shape = (64, 48, 7)
    per_slice = C.stars(shape, 3, n=50, reach=0.62)
    per_slice[3] = []
    per_slice[2].append(np.array([[-10.3, 24.3], [31.7, -9.6], [75.2, 23.1], [30.9, 60.4]]))     # a diamond through all four sides
    rng = np.random.default_rng(4)
    per_slice[5].append(C.star((100.2, 20.4), 8.0, 12, rng))                                    # wholly outside, right
    per_slice[5].append(C.star((-30.1, -29.7), 8.0, 12, rng))                                   # wholly outside, below and left
    arrays, want = _check(per_slice, shape)
    assert _outside(shape, arrays) and not want[:, :, 3].any() and want[:, :, 2].any()
    alone = C.arrays({5: per_slice[5][2:]}, shape[2])
    assert not _fill(alone, shape).any()
    nothing = C.arrays({}, shape[2])
    assert len(nothing[1]) == 0 and not _fill(nothing, shape).any()                              # n_contours == 0: every byte is still written


def test_unaligned_out():
    _check(C.stars((64, 6, 3), 1, n=12, reach=0.9), (64, 6, 3), out_lead=1)
    _check(C.stars((37, 29, 6), 1), (37, 29, 6), out_lead=7)


def test_rows_longer_than_one_workgroups_span():
    shape = (1040, 3, 2)
    arrays, want = _check({k: _wide_band(shape[0], k) for k in range(2)}, shape)
    assert want[1000:, :, :].any() and want[:16, :, :].any() and _outside(shape, arrays)
    _check({k: _wide_band(shape[0], k) for k in range(2)}, shape, out_lead=3)


def test_more_edges_than_one_chunk():
    n = _lib.RASTERIZE_CHUNK_EDGES + 37
    t = 0.3 + 2.0 * math.pi * np.arange(n) / n
    circle = np.stack([31.2 + 25.3 * np.cos(t), 30.7 + 25.3 * np.sin(t)], axis=1)
    inner = C.star((30.1, 31.9), 10.0, 31, np.random.default_rng(6))
    arrays, want = _check({0: [circle, inner]}, (64, 64, 1))
    assert arrays[1].tolist() == [[0, n], [n, 31]] and want[31, 8, 0] == 1 and want[30, 32, 0] == 0
    _check({0: [inner, circle]}, (64, 64, 1))                                                    # the chunk boundary falls elsewhere


def test_exact_lattice_case():
    """Vertices at integers and half-integers, axis-aligned and 45-degree edges: every operation is exact, the half-open rule decides."""
    shape = (12, 10, 1)
    poly = np.array([[2, 1], [2, 1], [9, 1], [9, 4], [11, 6], [9, 8], [5.5, 8], [2, 4.5]], dtype=np.float64)   # (2, 1) twice in a row
    arrays, want = _check({0: [poly]}, shape, exact=True)
    assert not want[:, 0, 0].any() and want[2:9, 1, 0].all() and not want[9:, 1, 0].any()        # a vertex on row 1: the row counts once
    assert want[2, 2, 0] == 1 and want[1, 2, 0] == 0                                             # a centre on the left edge is inside
    assert want[8, 2, 0] == 1 and want[9, 2, 0] == 0                                             # ... on the right edge outside
    assert want[:, 6, 0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0]                        # 45 degrees: xc = 3.5 and 11 at row 6
    assert want[:, 5, 0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0]                        # xc = 2.5 and 10 at row 5
    assert not want[:, 8, 0].any() and not want[:, 9, 0].any()                                   # the top edge is horizontal: never counts
    square = np.array([[3, 2], [7, 2], [7, 6], [3, 6]], dtype=np.float64)
    _check({0: [poly, square, square]}, shape, exact=True)                                       # a contour twice cancels itself


def test_order_of_contours_and_of_points_does_not_matter_and_two_calls_agree():
    shape = (64, 48, 7)
    per_slice = C.stars(shape, 3, n=50, reach=0.62)
    per_slice[2].append(np.array([[-10.3, 24.3], [31.7, -9.6], [75.2, 23.1], [30.9, 60.4]]))
    first = _fill(C.arrays(per_slice, shape[2]), shape)
    assert np.array_equal(first, _fill(C.arrays(per_slice, shape[2]), shape))
    rng = np.random.default_rng(9)
    shuffled = {k: [np.roll(polys[i], int(rng.integers(1, len(polys[i]))), axis=0) for i in rng.permutation(len(polys))] for k, polys in per_slice.items()}
    assert np.array_equal(first, _fill(C.arrays(shuffled, shape[2]), shape))
    # the records may also point anywhere into `points`: the same contours with the point blocks laid out in reverse
    points, records, slice_first = C.arrays(per_slice, shape[2])
    blocks = [points[f:f + c] for f, c in records][::-1]
    starts = np.cumsum([0] + [len(b) for b in blocks])[:-1][::-1]
    assert np.array_equal(first, _fill((np.concatenate(blocks), np.stack([starts, records[:, 1]], axis=1).astype(np.int32), slice_first), shape))


# ---- the NIfTI tree and its DICOM twin with RTSTRUCT masks through the collate ---------------------------------------------------------------
def _datasets(tree, **kw):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"], **kw)


def _with_geometry(ntree, n):
    """Every scan gets a geometry of its own, shared with its mask (the tree's is the identity)."""
    for i in range(n):
        for k, mod in enumerate(("t1", "t2")):
            d = os.path.join(ntree["image_loc"], mod, f"SYN-{i:04d}-{mod}-a")
            A = G.affine((("z", 0.05 + 0.01 * i), ("x", -0.03 * (k + 1))), (0.9, 0.8 + 0.1 * k, 3.0), (-40.5 + i, 22.25, -13.0 * (k + 1)))
            for name in (f"scan_{mod}.nii.gz", "mask.nii.gz"):
                img = nifti.read(os.path.join(d, name))
                nifti.write(os.path.join(d, name), img.raw, img.slope, img.inter, affine=A)


def test_twin_tree_with_rtstruct_masks_gives_the_same_batch(tmp_path):
    from mmnn_sts_amd.data import rtstruct
    ntree = synth_nifti.write_tree(tmp_path / "nifti", n_patients=4, seed=21, mask_grid="same")
    _with_geometry(ntree, 4)
    dtree = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / "dicom", seed=21, mask_format="rtstruct", extra_rois=("Body", "Marker"))
    a, b = _datasets(ntree), _datasets(dtree, mask_roi="gtv")
    assert (a.layout, b.layout) == ("nifti", "dicom") and a.uids == b.uids and len(a) == 4
    n, d = [a[i][0] for i in range(4)], [b[i][0] for i in range(4)]
    for p, q in zip(n, d):
        for (ns, nm), (s, m) in zip(p.volumes, q.volumes):
            assert isinstance(m, rtstruct.ContourSet) and m.names == ["GTV"] and s.shape == ns.shape == nm.shape
            # on the restatement alone: the contours give the NIfTI mask back, with every crossing half a voxel from a centre
            got, near_x, near_row = C.fill_ref(*rtstruct.to_scan_index(m, s.shape, s.affine)[:3], s.shape)
            assert near_x >= 0.49 and near_row >= 0.49 and np.array_equal(got, nm.raw != 0)
            assert ingest.mask_index_map(s, m) is None
    x_n, e_n = ingest.collate_volumes([p.volumes for p in n], DEV)
    x_d, e_d, kept = ingest.collate_volumes([p.volumes for p in d], DEV, keep_workspaces=True)
    torch.cuda.synchronize()
    assert x_n.shape == (4, 2, 64, 64, 64) and torch.equal(e_n, e_d) and int(e_n.min()) > 0
    assert torch.equal(x_n, x_d), f"{int((x_n != x_d).sum())} elements differ, max {float((x_n - x_d).abs().max())!r}"
    assert float(x_n.abs().max()) > 0.0
    assert kept[0][0].shape == d[0].volumes[0][0].shape and np.array_equal(kept[0][0].affine, d[0].volumes[0][0].affine)
    # the decoy ROI (the whole first slice) is another mask: selection is on the path
    x_o, _ = ingest.collate_volumes([p.volumes for p in [_datasets(dtree, mask_roi="Body")[0][0]]], DEV)
    assert not torch.equal(x_o[0], x_d[0])


def test_cli_trains_one_epoch_on_the_rtstruct_twin(tmp_path):
    ntree = synth_nifti.write_tree(tmp_path / "nifti", n_patients=4, seed=36, val_fraction=0.5)
    _with_geometry(ntree, 4)
    tree = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / "dicom", seed=36, mask_format="rtstruct", extra_rois=("Body",))
    log = run_main(["--images", "--survival", "--epochs", "1", "--config", tiny_config(tmp_path, data={"mask_roi": "GTV"}),
                    "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
                    "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]], tmp_path / "run", limit_s=600)
    assert "epoch 1/1" in log
