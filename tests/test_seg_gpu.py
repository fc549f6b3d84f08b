"""The DICOM SEG path on the device.  `mmnn_unpack_frames` against the numpy restatement of its contract (tests/_seg_ref.py), byte for
byte and with the output inside a patterned guard buffer; a synth_nifti tree against its synth_dicom twin with SEG masks through
`collate_volumes`, byte for byte, with the masks on the scans' grids and on grids of their own; and `main.py` on that twin in fresh
processes.

Byte-for-byte is a condition, not a tolerance: unpacking is integer arithmetic.  The own-grid twin then passes through the fp64 resample;
its seed is chosen on the CPU so that, on the restatement alone, no blend lies within 1e-6 * 128 of the threshold and no coordinate
within 1e-6 of the SEG volume's border under either index map, which the test asserts before it compares the batches."""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import ingest, nifti, seg, synth_dicom, synth_nifti
from tests import _resample_ref as G
from tests import _seg_ref as S
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
PATTERN = 0xA5


def _unpack(shape, bits, n_frames, refs, slice_first, one=1, out_lead=0, bits_lead=0, null=False):
    """The kernel's bytes as an (x, y, z) array through the C-ABI itself.  `out` sits inside a larger buffer whose other bytes must keep
    their pattern; `bits` starts `bits_lead` bytes into its buffer; `null`: bits and refs are passed as null pointers."""
    n = shape[0] * shape[1] * shape[2]
    lead = GUARD + out_lead
    buf = torch.full((lead + n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    stream = torch.from_numpy(np.frombuffer(b"\xFF" * bits_lead + bytes(bits) + b"\xFF" * 8, dtype=np.uint8).copy()).to(DEV)
    refs_d = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(refs, dtype=np.int32).reshape(-1), [0]]), dtype=np.int32)).to(DEV)
    first_d = torch.from_numpy(np.ascontiguousarray(slice_first, dtype=np.int32)).to(DEV)
    assert first_d.numel() == shape[2] + 1 and buf.data_ptr() % 256 == 0 and stream.data_ptr() % 256 == 0
    desc = _lib.UnpackFramesDesc(*shape, int(n_frames), len(refs), int(one))
    _lib.check(_lib.lib().mmnn_unpack_frames(ctypes.byref(desc), None if null else stream.data_ptr() + bits_lead, None if null else refs_d.data_ptr(),
                                             first_d.data_ptr(), buf.data_ptr() + lead, torch.cuda.current_stream().cuda_stream), "mmnn_unpack_frames")
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:lead] == PATTERN).all() and (b[lead + n:] == PATTERN).all(), "bytes outside `out` were written"
    return b[lead:lead + n].reshape(shape, order="F")


def _check(shape, planes, refs, slice_first, one=1, **kw):
    bits = S.pack_frames(planes)                                                         # the pad bits behind the last frame are all 1
    want = S.unpack_ref(bits, len(planes), refs, slice_first, shape, one)
    got = _unpack(shape, bits, len(planes), refs, slice_first, one, **kw)
    assert set(np.unique(got)) <= {0, one}
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{shape}: {bad.shape[0]} voxels differ, the first at {tuple(bad[0])}: device {got[tuple(bad[0])]}, restatement {want[tuple(bad[0])]}"
    return want


def _planes(shape, n, seed, density=0.5):
    return [(np.random.default_rng([seed, f]).random((shape[1], shape[0])) < density).astype(np.uint8) for f in range(n)]


def _one_per_slice(shape, seed, **kw):
    """Every slice has one frame, stored in a seeded order that is not the slices'."""
    z = shape[2]
    order = np.random.default_rng([seed, 99]).permutation(z)                             # frame order[k] belongs to slice k
    return _check(shape, _planes(shape, z, seed), order, np.arange(z + 1), **kw)


@pytest.mark.parametrize("one", [1, 255, 7])
def test_one_voxel(one):
    assert _check((1, 1, 1), [np.array([[1]])], [0], [0, 1], one).tolist() == [[[one]]]
    assert _check((1, 1, 1), [np.array([[0]])], [0], [0, 1], one).tolist() == [[[0]]]       # the stream's byte is 0xFE: seven pad bits set


def test_frames_that_start_in_the_middle_of_a_byte():
    want = _one_per_slice((5, 3, 4), 1)                                                  # bit starts 0, 15, 30, 45; the last frame ends at bit 60
    assert 0 < want.sum() < want.size
    _one_per_slice((7, 1, 9), 2)                                                         # 63 bits: one pad bit
    full = [np.ones((3, 5), dtype=np.uint8)] * 4
    assert _check((5, 3, 4), full, [3], [0, 0, 0, 1, 1]).sum() == 15                     # slices beside a full frame stay clear


def test_sparse_and_unordered_input():
    shape = (37, 29, 6)
    planes = _planes(shape, 5, 3, 0.3)                                                   # frames 1 and 3 are another segment's: never listed
    refs, first = [4, 2, 0], [0, 0, 2, 2, 2, 3, 3]                                       # slice 1: frames 4 and 2 OR-ed; slice 4: frame 0
    want = _check(shape, planes, refs, first)
    assert np.array_equal(want[:, :, 1], (planes[4] | planes[2]).T) and np.array_equal(want[:, :, 4], planes[0].T)
    assert not want[:, :, [0, 2, 3, 5]].any() and want[:, :, 1].sum() > planes[4].sum()
    ignored = _check(shape, planes, [4, 5, 2, -1, 0], [0, 0, 4, 4, 4, 5, 5])             # frame indices n_frames and -1 are ignored
    assert np.array_equal(ignored, want)
    # a frame may be listed for several slices; a slice range that does not lie inside refs is ignored as a whole
    several = _check(shape, planes, [0, 0, 1], [0, 1, 2, 3, 3, 3, 3])
    assert np.array_equal(several[:, :, 0], several[:, :, 1]) and several[:, :, 0].any()
    outside = _check(shape, planes, [0, 1], [0, 1, 2, 2, 7, 7, 1])                       # slices 3 .. 5: up to 7 > n_refs, 7 .. 7, 7 .. 1
    assert outside[:, :, :2].any() and not outside[:, :, 2:].any()
    for lead in (0, 5):                                                                  # n_refs == 0 with null pointers: every byte is still written
        assert not _unpack(shape, b"", 0, [], np.zeros(7, dtype=np.int32), out_lead=lead, null=True).any()
    assert not _check(shape, planes, [], np.zeros(7, dtype=np.int32)).any()


@pytest.mark.parametrize("shape,out_lead,bits_lead", [((64, 6, 3), 1, 1), ((64, 6, 3), 7, 3), ((37, 29, 6), 1, 3), ((37, 29, 6), 7, 1),
                                                      ((64, 6, 3), 0, 1), ((37, 29, 6), 0, 0)])
def test_unaligned_out_and_bits(shape, out_lead, bits_lead):
    assert _one_per_slice(shape, 4, out_lead=out_lead, bits_lead=bits_lead).any()


@pytest.mark.parametrize("out_lead", [0, 3])
def test_rows_longer_than_one_workgroups_span(out_lead):
    shape = (1040, 3, 2)                                                                 # x*y = 3120 = 16 * 195: no multiple of 8 * 16 either
    want = _one_per_slice(shape, 5, out_lead=out_lead)
    assert want[1030:, :, :].any() and want[:16, :, :].any()
    assert _check((1041, 3, 2), _planes((1041, 3, 2), 3, 6), [2, 0], [0, 1, 2], 255, out_lead=out_lead).any()     # x*y = 3123: no multiple of 16


def test_two_calls_agree_and_the_wrapper_gives_the_same_bytes():
    shape = (37, 29, 6)
    planes = _planes(shape, 6, 7)
    bits, refs, first = S.pack_frames(planes), [5, 0, 3, 1], [0, 1, 1, 3, 3, 4, 4]
    a, b = _unpack(shape, bits, 6, refs, first, 255), _unpack(shape, bits, 6, refs, first, 255)
    assert np.array_equal(a, b) and a.any()
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    v = ingest.unpack_frames((np.frombuffer(bits, dtype=np.uint8), 6, refs, first, 255), SimpleNamespace(shape=shape, affine=None), DEV, out=buf[GUARD:GUARD + n])
    torch.cuda.synchronize()
    assert v.datatype == 2 and (v.slope, v.inter) == (1.0, 0.0) and v.shape == shape and v.data.data_ptr() == buf.data_ptr() + GUARD and not v.from_dicom
    c = buf.cpu().numpy()
    assert (c[:GUARD] == PATTERN).all() and (c[GUARD + n:] == PATTERN).all() and np.array_equal(c[GUARD:GUARD + n].reshape(shape, order="F"), a)


# ---- the NIfTI tree and its DICOM twin with SEG masks through the collate ---------------------------------------------------------------
ON_GRID_SEED = 21
OWN_GRID_SEED = 50          # chosen on the CPU so that `_comparable` holds for every volume of the tree (a condition, not a tolerance)


def _datasets(tree, **kw):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"], **kw)


def _sparse_and_unordered(pairs):
    """The conditions the twin tests put on their trees: `pairs` = [(scan, FrameSet of the selected segment, Placement)]."""
    assert any((m.rows * m.columns) % 8 != 0 for _, m, _ in pairs), "no volume has frames that end inside a byte"
    assert any(len(p.refs) < p.shape[2] - (0 if p.on_scan else 2) for _, _, p in pairs), "no SEG omits an empty slice"
    assert any(p.refs.tolist() != sorted(p.refs.tolist()) for _, _, p in pairs), "every file stores its frames in slice order"


def test_twin_tree_with_seg_masks_on_the_scans_grids_gives_the_same_batch(tmp_path):
    from tests.test_rtstruct_gpu import _with_geometry
    ntree = synth_nifti.write_tree(tmp_path / "nifti", n_patients=4, seed=ON_GRID_SEED, mask_grid="same")
    _with_geometry(ntree, 4)
    dtree = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / "dicom", seed=ON_GRID_SEED, mask_format="seg", extra_rois=("Body", "Marker"))
    a, b = _datasets(ntree), _datasets(dtree, mask_roi="gtv")
    assert (a.layout, b.layout) == ("nifti", "dicom") and a.uids == b.uids and len(a) == 4 and b.other_grid == []
    n, d = [a[i][0] for i in range(4)], [b[i][0] for i in range(4)]
    pairs = []
    for p, q in zip(n, d):
        for (ns, nm), (s, m) in zip(p.volumes, q.volumes):
            assert isinstance(m, seg.FrameSet) and m.names == ["GTV"] and s.shape == ns.shape == nm.shape
            place = seg.to_scan(m, s.shape, s.affine)
            assert place.on_scan and place.one == 1 and ingest.mask_index_map(s, m) is None
            # on the restatement alone: the frames give the NIfTI mask back
            assert np.array_equal(S.unpack_ref(m.frame, m.n_frames, place.refs, place.slice_first, s.shape), (nm.raw != 0).astype(np.uint8))
            pairs.append((s, m, place))
    _sparse_and_unordered(pairs)
    x_n, e_n = ingest.collate_volumes([p.volumes for p in n], DEV)
    x_d, e_d, kept = ingest.collate_volumes([p.volumes for p in d], DEV, keep_workspaces=True)
    torch.cuda.synchronize()
    assert x_n.shape == (4, 2, 64, 64, 64) and torch.equal(e_n, e_d) and int(e_n.min()) > 0
    assert torch.equal(x_n, x_d), f"{int((x_n != x_d).sum())} elements differ, max {float((x_n - x_d).abs().max())!r}"
    assert float(x_n.abs().max()) > 0.0
    assert kept[0][0].shape == d[0].volumes[0][0].shape and np.array_equal(kept[0][0].affine, d[0].volumes[0][0].affine)
    # the decoy segment (the whole first slice) is another mask: selection is on the path
    x_o, _ = ingest.collate_volumes([p.volumes for p in [_datasets(dtree, mask_roi="Body")[0][0]]], DEV)
    assert not torch.equal(x_o[0], x_d[0])


def _own_grid_twins(root, seed):
    """(NIfTI patients, DICOM patients with SEG masks) of a tree whose masks lie on grids of their own, 0 / 255 on the NIfTI side."""
    ntree = synth_nifti.write_tree(os.path.join(root, "nifti"), n_patients=4, seed=seed, mask_grid="own")
    for mod in ("t1", "t2"):
        for p in sorted(os.listdir(os.path.join(ntree["image_loc"], mod))):
            path = os.path.join(ntree["image_loc"], mod, p, "mask.nii.gz")
            m = nifti.read(path)
            nifti.write(path, (m.raw * 255).astype(np.uint8), affine=m.affine)
    dtree = synth_dicom.from_nifti_tree(os.path.join(root, "nifti"), os.path.join(root, "dicom"), seed=seed, mask_format="seg")
    a, b = _datasets(ntree), _datasets(dtree)
    assert (a.layout, b.layout) == ("nifti", "dicom") and a.uids == b.uids and len(a) == 4 and len(b.other_grid) == 4
    return [a[i][0] for i in range(4)], [b[i][0] for i in range(4)]


def _comparable(nifti_patients, dicom_patients):
    """On the restatement alone (as `_comparable` of tests/test_dicom_gpu.py): under the NIfTI headers' index map into the whole mask
    volume and under the SEG elements' one into the stack of its frames, no blend lies within 1e-6 * 128 of the threshold and no
    coordinate within 1e-6 of a border of the mask's grid, and the two give the same bytes."""
    pairs = []
    for p, q in zip(nifti_patients, dicom_patients):
        for ch, ((ns, nm), (s, m)) in enumerate(zip(p.volumes, q.volumes)):
            assert ns.shape == s.shape and ns.shape != nm.shape and (m.columns, m.rows) == nm.shape[:2]
            place = seg.to_scan(m, s.shape, s.affine)
            chosen = place.refs
            step = float(m.steps[chosen[0]])
            shape, affine, slices = S.own_grid_ref(m.positions[chosen], m.orientations[chosen[0]], m.spacings[chosen[0]], step, m.rows, m.columns)
            assert not place.on_scan and place.one == 255 and place.shape == shape and np.abs(affine - place.affine).max() <= 1e-9
            refs, first = S.arrays(slices, chosen.tolist(), shape[2])
            assert np.array_equal(first, place.slice_first) and sorted(refs.tolist()) == sorted(place.refs.tolist())
            volume = S.unpack_ref(m.frame, m.n_frames, refs, first, shape, 255)
            assert not volume[:, :, 0].any() and not volume[:, :, -1].any() and volume[:, :, 1].any() and volume[:, :, -2].any()
            results = []
            for what, T, mask in (("nifti", G.index_map(ns.affine, nm.affine), nm.raw), ("seg", G.index_map(s.affine, affine), volume)):
                out, blend, c = G.resample_ref(mask, ns.shape, T, 128.0)
                G.assert_comparable(out, blend, c, mask.shape, 128.0, f"uid {p.uid} channel {ch} ({what} map)")
                value, edge = G.margins(out, blend, c, mask.shape, 128.0)
                assert value >= 1e-6 * 128.0, f"uid {p.uid} channel {ch} ({what} map): a blend lies within {value:.3e} of the threshold"
                assert edge >= 1e-6, f"uid {p.uid} channel {ch} ({what} map): a coordinate lies within {edge:.3e} of the mask grid's boundary"
                results.append(out)
            assert np.array_equal(*results) and results[0].any()
            pairs.append((s, m, place))
    return pairs


def test_twin_tree_with_seg_masks_on_their_own_grids_gives_the_same_batch(tmp_path):
    n, d = _own_grid_twins(str(tmp_path), OWN_GRID_SEED)
    _sparse_and_unordered(_comparable(n, d))
    x_n, e_n = ingest.collate_volumes([p.volumes for p in n], DEV, mask_threshold=128.0)
    x_d, e_d = ingest.collate_volumes([p.volumes for p in d], DEV)                        # unpacked at 255, resampled, binarised at 128
    torch.cuda.synchronize()
    assert x_n.shape == (4, 2, 64, 64, 64) and torch.equal(e_n, e_d) and int(e_n.min()) > 0
    assert torch.equal(x_n, x_d), f"{int((x_n != x_d).sum())} elements differ, max {float((x_n - x_d).abs().max())!r}"
    assert float(x_n.abs().max()) > 0.0


# ---- main.py on the SEG twin: fresh processes, one at a time -------------------------------------------------------------------------------
_main = functools.partial(run_main, limit_s=600)


def test_cli_trains_one_epoch_and_infers_in_scan_space_on_the_seg_twin(tmp_path):
    from mmnn_sts_amd.data import dicom
    from tests import _ingest_ref as R
    from tests.test_rtstruct_gpu import _with_geometry
    ntree = synth_nifti.write_tree(tmp_path / "nifti", n_patients=4, seed=36, val_fraction=0.5)
    _with_geometry(ntree, 4)
    tree = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / "dicom", seed=36, mask_format="seg", extra_rois=("Body",))
    cfg = tiny_config(tmp_path, data={"mask_roi": "GTV"})
    loc = ["--config", cfg, "--image_loc", tree["image_loc"], "--key_loc", tree["key_loc"], "--data_loc", tree["data_loc"],
           "--train_uid_location", tree["train_uids"], "--val_uid_location", tree["val_uids"]]
    out = tmp_path / "run"
    out.mkdir()
    log = _main(["--images", "--preop", "--survival", "--blend", "--transforms", "--epochs", "1", *loc], out)
    assert "epoch 1/1" in log
    log = _main(["--inference", "--images", "--preop", "--survival", "--transforms", "--scan_space", "--weights", str(out / "best_surv_model.pth"), *loc], out)
    assert "All C-indexes" in log
    val_uids = [int(l) for l in open(tree["val_uids"]).read().split()]
    index = {uid: i for i, uid in enumerate(ntree["uids"])}
    for uid in val_uids:
        series = dicom.read_series(os.path.join(tree["image_loc"], "t1", f"SYN-{index[uid]:04d}-t1-a", "image"), header_only=True)
        h = R.read_nifti_file(out / "attention_maps" / f"_patient_{uid}" / "att_map_class0_on_t1.nii.gz")
        assert h["dim"][:4] == (3, *series.shape) and np.isfinite(h["data"]).all()
