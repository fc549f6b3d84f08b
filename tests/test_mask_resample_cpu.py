"""`not gpu` tests of the mask-resample feature's host side: the geometry the NIfTI reader and writer now carry (against the published
offsets, parsed and packed by tests/_resample_ref.py), `nifti.index_map`, the synthetic tree with masks on grids of their own, the
datasets' acceptance / refusal of such patients, the `Data:` keys, and the library's refusals (pure host checks)."""
import ctypes
import filecmp
import logging
import os
import types

import numpy as np
import pytest

from mmnn_sts_amd.data import nifti, synth_nifti
from mmnn_sts_amd.data.ImageDatasets import NiftiSurvivalDataset, T1T2SurvivalDataset
from mmnn_sts_amd.data.ingest import RawPatient
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from mmnn_sts_amd.parser.parser import Parser
from tests import _ingest_ref as R
from tests import _resample_ref as G

EXTENT = ((12, 20), (12, 20), (8, 12))


# ---- reader / writer ---------------------------------------------------------------------------------------------------------------
def test_written_affine_reads_back_to_float32_rounding(tmp_path):
    A = G.affine((("z", 0.21), ("x", -0.13)), (1.7, 1.3, 2.9), (-9.3, -12.1, -17.7))
    a = np.arange(4 * 5 * 6, dtype=np.int16).reshape(4, 5, 6)
    for name in ("v.nii", "v.nii.gz"):
        p = nifti.write(tmp_path / name, a, 0.5, 1.0, affine=A)
        img = nifti.read(p)
        assert img.affine.dtype == np.float64 and img.affine.shape == (4, 4)
        assert np.array_equal(img.affine[:3], A[:3].astype(np.float32).astype(np.float64)) and np.array_equal(img.affine[3], [0, 0, 0, 1])
        assert np.array_equal(img.raw, a) and (img.slope, img.inter) == (0.5, 1.0)
        buf = G.file_bytes(p)
        assert np.array_equal(G.parse_affine(buf), img.affine)                              # the same srow bytes, parsed by struct
        h = R.parse_nifti(buf)
        assert h["sform_code"] == 2 and np.array_equal(h["srow"], A[:3].astype(np.float32).astype(np.float64))
        assert nifti.read_geometry(p)[0] == (4, 5, 6) and np.array_equal(nifti.read_geometry(p)[1], img.affine)
    assert np.array_equal(nifti.read(nifti.write(tmp_path / "plain.nii", a)).affine, np.eye(4))
    with pytest.raises(ConfigurationError):
        nifti.write(tmp_path / "bad.nii", a, affine=np.full((4, 4), np.nan))


@pytest.mark.parametrize("qfac", [1.0, -1.0, 0.0])
@pytest.mark.parametrize("bo", ["<", ">"])
def test_qform_reads_back_as_the_quaternion_formula(tmp_path, qfac, bo):
    quatern, qoffset, spacing = (0.12, -0.31, 0.47), (-91.5, 102.25, -33.0), (0.8, 0.9, 3.2)
    raw = np.zeros((3, 4, 5), dtype=np.uint8)
    (tmp_path / "q.nii").write_bytes(G.pack_geometry(raw, 2, qform=(1, quatern, qoffset, (qfac, *spacing)), byteorder=bo))
    got = nifti.read(tmp_path / "q.nii").affine
    q32 = [float(np.float32(v)) for v in quatern]
    want = np.eye(4)
    want[:3, :3] = G.quaternion_rotation(*q32) * np.array([np.float32(s) for s in spacing], dtype=np.float64) * np.array([1.0, 1.0, -1.0 if qfac < 0 else 1.0])
    want[:3, 3] = [np.float32(v) for v in qoffset]
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert np.allclose(got[:3, :3].T @ got[:3, :3], np.diag(np.square(want[:3, :3]).sum(axis=0)), atol=1e-5)      # orthogonal columns
    assert np.sign(np.linalg.det(got[:3, :3])) == (-1.0 if qfac < 0 else 1.0)
    assert np.array_equal(got, G.parse_affine(G.file_bytes(tmp_path / "q.nii"), bo))


def test_sform_wins_over_qform_and_no_codes_means_no_geometry(tmp_path):
    raw = np.zeros((3, 4, 5), dtype=np.uint8)
    rows = G.affine((("y", 0.3),), (2.0, 1.0, 0.5), (1.0, 2.0, 3.0))
    q = (1, (0.1, 0.2, 0.3), (5.0, 6.0, 7.0), (1.0, 1.0, 1.0, 1.0))
    (tmp_path / "both.nii").write_bytes(G.pack_geometry(raw, 2, qform=q, sform=(1, rows)))
    assert np.array_equal(nifti.read(tmp_path / "both.nii").affine[:3], rows[:3].astype(np.float32).astype(np.float64))
    (tmp_path / "none.nii").write_bytes(G.pack_geometry(raw, 2))
    assert nifti.read(tmp_path / "none.nii").affine is None and nifti.read_geometry(tmp_path / "none.nii") == ((3, 4, 5), None)
    (tmp_path / "zero.nii").write_bytes(G.pack_geometry(raw, 2, qform=(0, q[1], q[2], q[3]), sform=(0, rows)))       # fields set, codes 0
    assert nifti.read(tmp_path / "zero.nii").affine is None


def test_file_without_affine_is_byte_identical_to_the_earlier_layout(tmp_path):
    a = (np.arange(5 * 6 * 7).reshape(5, 6, 7) % 251).astype(np.int16)
    assert nifti.header_bytes((5, 6, 7), 4, 0.25, -12.5) == G.identity_header((5, 6, 7), 4, 0.25, -12.5)
    assert nifti.header_bytes((5, 6, 7), 4, 0.25, -12.5, affine=None) == G.identity_header((5, 6, 7), 4, 0.25, -12.5)
    p = nifti.write(tmp_path / "a.nii", a, 0.25, -12.5)
    assert open(p, "rb").read() == G.identity_header((5, 6, 7), 4, 0.25, -12.5) + a.astype("<i2").tobytes(order="F")
    assert G.file_bytes(nifti.write(tmp_path / "a.nii.gz", a, 0.25, -12.5)) == open(p, "rb").read()
    img = nifti.NiftiImage(a, 4, 1.0, 0.0, "somewhere")                                     # positional construction as before
    assert img.path == "somewhere" and img.affine is None


# ---- index_map -----------------------------------------------------------------------------------------------------------------------
def test_index_map_is_inverse_mask_affine_times_scan_affine():
    _, _, SA, MA, T = G.case("E")
    scan = nifti.NiftiImage(np.zeros((2, 2, 2), np.uint8), 2, 1.0, 0.0, "scan_t1.nii.gz", SA)
    mask = nifti.NiftiImage(np.zeros((2, 2, 2), np.uint8), 2, 1.0, 0.0, "mask.nii.gz", MA)
    got = nifti.index_map(scan, mask)
    assert got.shape == (3, 4) and got.dtype == np.float64 and np.abs(got - T).max() <= 1e-12 * np.abs(T).max()
    p = np.array([7.0, 3.0, 2.0, 1.0])
    assert np.allclose(MA[:3, :3] @ (got @ p) + MA[:3, 3], (SA @ p)[:3], atol=1e-9)          # both name the same point in space
    mask.affine = None
    with pytest.raises(ConfigurationError, match="mask.nii.gz"):
        nifti.index_map(scan, mask)
    mask.affine = MA.copy()
    mask.affine[:3, 2] = 2.0 * mask.affine[:3, 1]
    with pytest.raises(ConfigurationError, match="mask.nii.gz.*singular"):
        nifti.index_map(scan, mask)
    scan.affine = None
    with pytest.raises(ConfigurationError, match="scan_t1.nii.gz"):
        nifti.index_map(scan, mask)


def test_mask_index_map_modes():
    from mmnn_sts_amd.data import ingest
    _, _, SA, MA, T = G.case("A")
    vol = lambda shape, A: types.SimpleNamespace(shape=shape, affine=A, path="")
    assert ingest.mask_index_map(vol((20, 18, 16), None), vol((20, 18, 16), None), "auto") is None
    assert ingest.mask_index_map(vol((20, 18, 16), SA), vol((20, 18, 16), MA), "auto") is None          # equal extents: as before
    assert np.allclose(ingest.mask_index_map(vol((20, 18, 16), SA), vol((13, 17, 11), MA), "auto"), T)
    assert np.allclose(ingest.mask_index_map(vol((20, 18, 16), SA), vol((20, 18, 16), MA), "geometry"), T)
    assert ingest.mask_index_map(vol((20, 18, 16), SA), vol((20, 18, 16), SA.copy()), "geometry") is None
    assert ingest.mask_index_map(vol((20, 18, 16), SA), vol((20, 18, 16), None), "geometry") is None
    shifted = SA.copy()
    shifted[:3, 3] += SA[:3, :3] @ [2e-3, 0.0, 0.0]                                          # 2e-3 voxel along x: above the 1e-3 rule
    assert ingest.mask_index_map(vol((20, 18, 16), SA), vol((20, 18, 16), shifted), "geometry") is not None
    shifted = SA.copy()
    shifted[:3, 3] += SA[:3, :3] @ [5e-4, 0.0, 0.0]
    assert ingest.mask_index_map(vol((20, 18, 16), SA), vol((20, 18, 16), shifted), "geometry") is None
    with pytest.raises(ConfigurationError, match="never"):
        ingest.mask_index_map(vol((20, 18, 16), SA), vol((13, 17, 11), MA), "never")
    with pytest.raises(ConfigurationError):
        ingest.mask_index_map(vol((20, 18, 16), SA), vol((13, 17, 11), None), "auto")
    with pytest.raises(ConfigurationError):
        ingest.mask_index_map(vol((20, 18, 16), SA), vol((13, 17, 11), MA), "sometimes")


# ---- the synthetic tree ------------------------------------------------------------------------------------------------------------
def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_default_tree_is_unchanged_and_own_grid_masks_differ(tmp_path):
    a = synth_nifti.write_tree(tmp_path / "a", n_patients=3, seed=3, extent=EXTENT)
    b = synth_nifti.write_tree(tmp_path / "b", n_patients=3, seed=3, extent=EXTENT, mask_grid="same")
    c = synth_nifti.write_tree(tmp_path / "c", n_patients=3, seed=3, extent=EXTENT, mask_grid="own")
    names = _files(tmp_path / "a")
    assert names == _files(tmp_path / "b") == _files(tmp_path / "c") and len(names) == 3 * 2 * 2 + 4
    for n in names:
        assert filecmp.cmp(tmp_path / "a" / n, tmp_path / "b" / n, shallow=False), n
    # the default tree is the one written before masks could have a grid of their own: identity sform, scan and mask on one grid
    for mod in ("t1", "t2"):
        for d in sorted(os.listdir(os.path.join(a["image_loc"], mod))):
            scan = G.file_bytes(os.path.join(a["image_loc"], mod, d, f"scan_{mod}.nii.gz"))
            shape = R.parse_nifti(scan)["dim"][1:4]
            assert scan[:352] == G.identity_header(shape, 4, synth_nifti.SCAN_SLOPE, synth_nifti.SCAN_INTER)
            assert G.file_bytes(os.path.join(a["image_loc"], mod, d, "mask.nii.gz"))[:352] == G.identity_header(shape, 2)
            # 'own': the same scan voxels under another affine; the mask on other extents along every axis, with an affine of its own
            own_scan = nifti.read(os.path.join(c["image_loc"], mod, d, f"scan_{mod}.nii.gz"))
            own_mask = nifti.read(os.path.join(c["image_loc"], mod, d, "mask.nii.gz"))
            assert np.array_equal(own_scan.raw, R.parse_nifti(scan)["data"])
            assert all(m != s for m, s in zip(own_mask.shape, own_scan.shape)) and own_mask.raw.any()
            assert not np.allclose(own_scan.affine, np.eye(4)) and not np.allclose(own_mask.affine, own_scan.affine)
            assert set(np.unique(own_mask.raw)) <= {0, 1}
    for k in ("key_loc", "data_loc", "train_uids", "val_uids"):
        assert filecmp.cmp(a[k], c[k], shallow=False)
    with pytest.raises(ValueError):
        synth_nifti.write_tree(tmp_path / "d", n_patients=1, mask_grid="other")


# ---- datasets and config -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def own_tree(tmp_path_factory):
    return synth_nifti.write_tree(tmp_path_factory.mktemp("own"), n_patients=3, seed=5, extent=EXTENT, mask_grid="own")


def _t1t2(tree, **kw):
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"], **kw)


def test_own_grid_tree_constructs_and_yields_raw_patients(own_tree, caplog):
    with caplog.at_level(logging.INFO, logger="mmnn_sts_amd"):
        ds = _t1t2(own_tree)
    said = [r.getMessage() for r in caplog.records if "another grid" in r.getMessage()]
    assert len(said) == 2 and all(s.startswith("3 of 3 patients") for s in said) and "t1" in said[0] and "t2" in said[1]      # once per tree
    assert len(ds) == 3
    raw, events, durations = ds[1]
    assert isinstance(raw, RawPatient) and raw.uid == own_tree["uids"][1] and len(raw.volumes) == 2
    for scan, mask in raw.volumes:
        assert scan.shape != mask.shape and scan.affine is not None and mask.affine is not None
        T = nifti.index_map(scan, mask)
        want = G.index_map(G.parse_affine(G.file_bytes(scan.path)), G.parse_affine(G.file_bytes(mask.path)))
        assert np.abs(T - want).max() <= 1e-12 * np.abs(want).max()
        out, m, c = G.resample_ref(mask.raw, scan.shape, want)                               # the tree is usable: the mask lands in the scan
        assert 0 < out.sum() < out.size


def test_same_grid_tree_says_nothing(tmp_path, caplog):
    tree = synth_nifti.write_tree(tmp_path, n_patients=2, seed=6, extent=EXTENT)
    with caplog.at_level(logging.INFO, logger="mmnn_sts_amd"):
        ds = _t1t2(tree)
    assert not [r for r in caplog.records if "another grid" in r.getMessage()] and ds.t1_dataset.other_grid == []


def test_own_grid_without_geometry_or_with_never_is_refused(tmp_path):
    tree = synth_nifti.write_tree(tmp_path, n_patients=2, seed=7, extent=EXTENT, modalities=("t1",), mask_grid="own")
    t1 = os.path.join(tree["image_loc"], "t1")
    assert len(NiftiSurvivalDataset(t1, tree["data_loc"], tree["key_loc"])) == 2
    with pytest.raises(ConfigurationError, match=r"SYN-0000-t1-a.*scan extent.*mask extent.*never"):
        NiftiSurvivalDataset(t1, tree["data_loc"], tree["key_loc"], mask_resample="never")
    with pytest.raises(ConfigurationError, match="mask_resample"):
        NiftiSurvivalDataset(t1, tree["data_loc"], tree["key_loc"], mask_resample="sometimes")
    G.strip_geometry(os.path.join(t1, "SYN-0001-t1-a", "mask.nii.gz"))
    with pytest.raises(ConfigurationError, match=r"SYN-0001-t1-a.*mask.nii.gz has no qform/sform to resample by"):
        NiftiSurvivalDataset(t1, tree["data_loc"], tree["key_loc"])
    for d in sorted(os.listdir(t1)):
        for f in os.listdir(os.path.join(t1, d)):
            G.strip_geometry(os.path.join(t1, d, f))
    with pytest.raises(ConfigurationError, match=rf"SYN-0000-t1-a \(uid {tree['uids'][0]}\): scan extent .* mask extent .* and neither file has a qform/sform to resample by"):
        NiftiSurvivalDataset(t1, tree["data_loc"], tree["key_loc"])


def test_data_keys_reach_the_datasets_and_the_collate(own_tree):
    args = types.SimpleNamespace(images=True, preop=False, postop=False, survival=True, classification=False,
                                 image_loc=own_tree["image_loc"], data_loc=own_tree["data_loc"], key_loc=own_tree["key_loc"])
    p = Parser(None)
    p.parseConfig()
    p.applyDataFlags(args)
    assert p.maskResample() == ("auto", 0.5)
    assert p.getDatasets(args, p.getImagePath()).mask_resample == "auto"
    p.config["Data"].update(mask_resample="geometry", mask_threshold=128)
    assert p.maskResample() == ("geometry", 128.0)
    ds = p.getDatasets(args, p.getImagePath())
    assert ds.mask_resample == ds.t1_dataset.mask_resample == ds.t2_dataset.mask_resample == "geometry"
    p.config["Data"]["mask_resample"] = "never"
    with pytest.raises(ConfigurationError, match="never"):
        p.getDatasets(args, p.getImagePath())
    p.config["Data"]["mask_resample"] = "always"
    with pytest.raises(ConfigurationError, match="mask_resample"):
        p.maskResample()
    p.config["Data"].update(mask_resample="auto", mask_threshold="half")
    with pytest.raises(ConfigurationError, match="mask_threshold"):
        p.maskResample()


# ---- the library's refusals (host checks, no GPU) ----------------------------------------------------------------------------------
def test_resample_mask_error_contract():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    ident = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def status(x=8, y=8, z=8, mx=4, my=4, mz=4, code=2, T=ident, thr=0.5):
        d = _lib.ResampleMaskDesc(x, y, z, mx, my, mz, code, 1.0, 0.0, (ctypes.c_double * 12)(*T), thr)
        return L.mmnn_resample_mask(ctypes.byref(d), None, None, None), _lib.last_error()

    assert ctypes.sizeof(_lib.ResampleMaskDesc) == 144 and _lib.ResampleMaskDesc.index_map.offset == 40
    for kw, word in ((dict(y=0), "extent"), (dict(mz=-3), "extent"), (dict(x=2048, y=2048, z=512), "2^31"), (dict(mx=1290, my=1290, mz=1291), "2^31"),
                     (dict(code=128), "datatype code 128"), (dict(T=ident[:5] + [float("nan")] + ident[6:]), "index_map[5]"),
                     (dict(T=[float("inf")] + ident[1:]), "index_map[0]"), (dict(thr=float("nan")), "threshold"), (dict(thr=float("-inf")), "threshold"),
                     (dict(), "null argument")):
        st, msg = status(**kw)
        assert st == 1 and word in msg, (kw, st, msg)
    assert L.mmnn_resample_mask(None, None, None, None) == 1
