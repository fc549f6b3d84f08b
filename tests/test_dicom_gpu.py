"""The DICOM path on the device.  `mmnn_decode_slices` against the numpy restatement of its contract (tests/_dicom_ref.py), bit for bit,
with the output inside a patterned guard buffer; a synth_nifti tree against its synth_dicom twin through `collate_volumes`, byte for
byte (derived, not measured: the decode is exact integer work, the shared slope is applied by the same ingest code, and the ingest is
deterministic); and `main.py` on the twin in fresh processes."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib
from mmnn_sts_amd.data import dicom, ingest, nifti, synth_dicom, synth_nifti
from tests import _dicom_ref as D
from tests import _ingest_ref as R
from tests import _resample_ref as G
from tests._cli import run_main, tiny_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
PATTERN = 0xA5

# (bits_allocated, bits_stored, high_bit, is_signed)
TYPES = {"u8": (8, 8, 7, 0), "i8": (8, 8, 7, 1), "u16": (16, 16, 15, 0), "i16": (16, 16, 15, 1), "i32": (32, 32, 31, 1), "u32": (32, 32, 31, 0),
         "i16_12_stored": (16, 12, 11, 1), "u16_12_stored": (16, 12, 11, 0), "i16_12_stored_high_bit_13": (16, 12, 13, 1)}
# (extent, pixel offset in elements, extra out offset in elements): the last but one has rows of a multiple of 16 bytes in buffers that
# start one element off; the last spans more than one block along x in every vector path, with a partial last group
EXTENTS = [((1, 1, 1), 0, 0), ((5, 3, 2), 0, 0), ((33, 17, 5), 0, 0), ((64, 48, 7), 0, 0), ((64, 6, 3), 1, 1), ((1040, 3, 2), 0, 0)]


def _words(shape, bits, seed):
    """Random words over the whole range of the stored type: the unused bits hold garbage."""
    return np.random.default_rng(seed).integers(0, 1 << bits, shape, dtype=np.uint64).astype(f"u{bits // 8}")


def _scales(z):
    return np.array([[0.37 + 0.11 * k, -1000.5 + 3.0 * k] for k in range(z)], dtype=np.float64)     # fractional slopes, negative intercepts


def _decode(words, kind, scale=None, pixel_lead=0, out_lead=0):
    """The kernel's output bytes; `out` sits inside a larger buffer whose other bytes must keep their pattern."""
    bits, stored, high, signed = TYPES[kind]
    x, y, z = words.shape
    isz, osz = bits // 8, (8 if scale is not None else bits // 8)
    raw = np.frombuffer(words.astype(words.dtype.newbyteorder("<")).tobytes(order="F"), dtype=np.uint8)
    pixels = torch.empty(pixel_lead * isz + raw.size, dtype=torch.uint8, device=DEV)
    pixels[pixel_lead * isz:] = torch.from_numpy(raw.copy()).to(DEV)
    table = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale)).to(DEV)
    lead, n = GUARD + out_lead * osz, words.size * osz
    buf = torch.full((lead + n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    code = 64 if scale is not None else D.INTEGER_CODE[bits, signed]
    desc = _lib.DecodeSlicesDesc(x, y, z, bits, stored, high, signed, code)
    _lib.check(_lib.lib().mmnn_decode_slices(ctypes.byref(desc), pixels.data_ptr() + pixel_lead * isz, None if table is None else table.data_ptr(),
                                             buf.data_ptr() + lead, torch.cuda.current_stream().cuda_stream), "mmnn_decode_slices")
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:lead] == PATTERN).all() and (b[lead + n:] == PATTERN).all(), "bytes outside `out` were written"
    return b[lead:lead + n].tobytes(), code


@pytest.mark.parametrize("kind", sorted(TYPES))
def test_decode_equals_the_restatement_bit_for_bit(kind):
    bits, stored, high, signed = TYPES[kind]
    for n, (shape, pixel_lead, out_lead) in enumerate(EXTENTS):
        words = _words(shape, bits, 100 + n)
        for scale in (None, _scales(shape[2])):
            want = D.decode_ref(words, stored, high, bool(signed), scale)
            got, code = _decode(words, kind, scale, pixel_lead, out_lead)
            assert want.dtype == np.dtype(D.NP_OF_CODE[code].lstrip("<"))
            got = np.frombuffer(got, dtype=D.NP_OF_CODE[code]).reshape(shape, order="F")
            bad = np.argwhere(got.view(f"u{got.dtype.itemsize}") != want.view(f"u{want.dtype.itemsize}"))
            assert bad.shape[0] == 0, (f"{kind} {shape} {'float64' if scale is not None else 'integer'}: {bad.shape[0]} voxels differ, the first at "
                                       f"{tuple(bad[0])}: word {int(words[tuple(bad[0])]):#x}, device {got[tuple(bad[0])]!r}, restatement {want[tuple(bad[0])]!r}")
            if scale is None and stored < bits:
                assert not np.array_equal(want.view(words.dtype), words)                    # the garbage was there to be dropped


def test_two_calls_give_identical_bytes():
    for kind, (shape, pixel_lead, out_lead) in (("i16_12_stored", EXTENTS[3]), ("u8", EXTENTS[4]), ("i32", EXTENTS[5])):
        words = _words(shape, TYPES[kind][0], 7)
        for scale in (None, _scales(shape[2])):
            assert _decode(words, kind, scale, pixel_lead, out_lead)[0] == _decode(words, kind, scale, pixel_lead, out_lead)[0]


def test_decode_series_picks_the_output_type(tmp_path):
    vol = np.random.default_rng(8).integers(-2048, 2048, (12, 9, 5)).astype("i2")
    for sub, kw, want_type, want_scale in (("u", dict(slope=0.25, inter=-12.5), 4, (0.25, -12.5)), ("p", dict(slope=0.25, inter=-12.5, per_slice_scale=True), 64, (1.0, 0.0)),
                                           ("w", dict(slope=0.1, inter=0.0), 64, (1.0, 0.0)), ("b", dict(bits_stored=12), 4, (1.0, 0.0))):
        synth_dicom.write_series(tmp_path / sub, vol, **kw)
        series = dicom.read_series(tmp_path / sub)
        v = ingest.upload(series, DEV)
        torch.cuda.synchronize()
        assert v.from_dicom and v.shape == vol.shape and v.datatype == want_type and (v.slope, v.inter) == want_scale and v.affine is series.affine
        got = np.frombuffer(v.data.cpu().numpy().tobytes(), dtype=D.NP_OF_CODE[want_type]).reshape(vol.shape, order="F")
        if want_type == 4:
            assert np.array_equal(got, vol)
        else:                                   # 0.1 is not a float32: the ingest's descriptor could not carry it, so the kernel applies it
            assert np.array_equal(got, vol.astype(np.float64) * np.asarray(series.slopes)[None, None] + np.asarray(series.inters)[None, None])
    with pytest.raises(ValueError, match="header_only"):
        ingest.upload(dicom.read_series(tmp_path / "u", header_only=True), DEV)


# ---- the NIfTI tree and its DICOM twin through the collate -----------------------------------------------------------------------------
OWN_GRID_SEED = 50          # chosen on the CPU so that `_comparable` holds for every volume of the tree (a condition, not a tolerance)


def _datasets(tree):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])


def _twins(tmp_path, seed, mask_grid="same", **kw):
    n = synth_nifti.write_tree(tmp_path / "nifti", n_patients=4, seed=seed, mask_grid=mask_grid)
    if mask_grid == "own":                      # 0 / 255 masks on both sides
        for mod in ("t1", "t2"):
            for p in sorted(os.listdir(os.path.join(n["image_loc"], mod))):
                path = os.path.join(n["image_loc"], mod, p, "mask.nii.gz")
                m = nifti.read(path)
                nifti.write(path, (m.raw * 255).astype(np.uint8), affine=m.affine)
    d = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / "dicom", mask_value=255, shuffle_names=True, seed=seed, **kw)
    a, b = _datasets(n), _datasets(d)
    assert (a.layout, b.layout) == ("nifti", "dicom") and a.uids == b.uids and len(a) == 4
    return [a[i][0] for i in range(4)], [b[i][0] for i in range(4)]


def _assert_equal_batches(nifti_patients, dicom_patients, nifti_threshold):
    x_n, e_n = ingest.collate_volumes([p.volumes for p in nifti_patients], DEV, mask_threshold=nifti_threshold)
    x_d, e_d = ingest.collate_volumes([p.volumes for p in dicom_patients], DEV)                # a DICOM pair: resampled, at 128
    torch.cuda.synchronize()
    assert x_n.shape == (4, 2, 64, 64, 64) and torch.equal(e_n, e_d) and int(e_n.min()) > 0
    assert torch.equal(x_n, x_d), f"{int((x_n != x_d).sum())} elements differ, max {float((x_n - x_d).abs().max())!r}"
    assert float(x_n.abs().max()) > 0.0
    return x_n


def test_twin_trees_give_equal_batches(tmp_path):
    n, d = _twins(tmp_path, 21)
    for p, q in zip(n, d):
        for (ns, nm), (s, m) in zip(p.volumes, q.volumes):
            assert ns.raw.dtype == np.int16 and (ns.slope, ns.inter) == (0.25, -12.5) == s.uniform_scale() and set(np.unique(nm.raw)) == {0, 1}
            assert s.shape == ns.shape == m.shape and [os.path.basename(f) for f in s.files] != sorted(os.path.basename(f) for f in s.files)
    _assert_equal_batches(n, d, 0.5)


def test_twin_with_per_slice_scales_equals_the_float64_nifti(tmp_path):
    n, d = _twins(tmp_path, 22, per_slice_scale=True)
    scaled = []
    for p, q in zip(n, d):
        volumes = []
        for (ns, nm), (s, _) in zip(p.volumes, q.volumes):
            assert s.uniform_scale() is None and len(set(s.slopes)) == min(4, s.shape[2]) and min(s.inters) < 0
            values = ns.raw.astype(np.float64) * np.asarray(s.slopes)[None, None, :] + np.asarray(s.inters)[None, None, :]
            volumes.append((nifti.NiftiImage(values, 64, 1.0, 0.0, ns.path, ns.affine), nm))
        scaled.append(ingest.RawPatient(p.uid, volumes))
    _assert_equal_batches(scaled, d, 0.5)


def _comparable(nifti_patients, dicom_patients):
    """On the restatement alone: under the NIfTI headers' index map and under the DICOM elements' one, no blend lies within 1e-6 * 128 of
    the threshold and no coordinate within 1e-6 of a border of the mask's grid, and the two give the same bytes."""
    for p, q in zip(nifti_patients, dicom_patients):
        for ch, ((ns, nm), (s, m)) in enumerate(zip(p.volumes, q.volumes)):
            assert ns.shape == s.shape and nm.shape == m.shape and ns.shape != nm.shape
            results = []
            for what, T in (("nifti", G.index_map(ns.affine, nm.affine)), ("dicom", G.index_map(s.affine, m.affine))):
                out, blend, c = G.resample_ref(nm.raw, ns.shape, T, 128.0)
                G.assert_comparable(out, blend, c, nm.shape, 128.0, f"uid {p.uid} channel {ch} ({what} map)")
                value, edge = G.margins(out, blend, c, nm.shape, 128.0)
                assert value >= 1e-6 * 128.0, f"uid {p.uid} channel {ch} ({what} map): a blend lies within {value:.3e} of the threshold"
                assert edge >= 1e-6, f"uid {p.uid} channel {ch} ({what} map): a coordinate lies within {edge:.3e} of the mask grid's boundary"
                results.append(out)
            assert np.array_equal(*results)


def test_twin_trees_with_masks_on_their_own_grids(tmp_path):
    n, d = _twins(tmp_path, OWN_GRID_SEED, mask_grid="own")
    _comparable(n, d)
    _assert_equal_batches(n, d, 128.0)


# ---- main.py on the DICOM twin: fresh processes, one at a time ---------------------------------------------------------------------------
_main = functools.partial(run_main, limit_s=600)


def _epoch_line(log):
    lines = re.findall(r"epoch 1/1 .*", log)
    assert len(lines) == 1, log[-2000:]
    return lines[0]


def test_cli_trains_and_infers_on_the_dicom_twin(tmp_path):
    from mmnn_sts_amd.models.densenet import TinyDensenet
    from mmnn_sts_amd.models.multimodal import MultiModalModel
    ntree = synth_nifti.write_tree(tmp_path / "nifti", n_patients=4, seed=35, val_fraction=0.5)
    # every scan gets a geometry of its own, shared with its mask (the tree's is the identity, which a writer that forgot the affine would emit too)
    for i in range(4):
        for k, mod in enumerate(("t1", "t2")):
            d = os.path.join(ntree["image_loc"], mod, f"SYN-{i:04d}-{mod}-a")
            A = G.affine((("z", 0.05 + 0.01 * i), ("x", -0.03 * (k + 1))), (0.9, 0.8 + 0.1 * k, 3.0), (-40.5 + i, 22.25, -13.0 * (k + 1)))
            for name in (f"scan_{mod}.nii.gz", "mask.nii.gz"):
                img = nifti.read(os.path.join(d, name))
                nifti.write(os.path.join(d, name), img.raw, img.slope, img.inter, affine=A)
    tree = synth_dicom.from_nifti_tree(tmp_path / "nifti", tmp_path / "dicom", seed=35)
    cfg = tiny_config(tmp_path)
    loc = lambda t: ["--config", cfg, "--image_loc", t["image_loc"], "--key_loc", t["key_loc"], "--data_loc", t["data_loc"],
                     "--train_uid_location", t["train_uids"], "--val_uid_location", t["val_uids"]]
    train = ["--images", "--preop", "--survival", "--blend", "--transforms", "--epochs", "1"]
    out = tmp_path / "dicom_run"
    out.mkdir()
    log = _main([*train, *loc(tree)], out)
    img = TinyDensenet(spatial_dims=3, in_channels=2, out_channels=2, feature_channels=12, dropout_prob=0.2)
    MultiModalModel(img, [f"p{i}" for i in range(32)], 2, 12, blend=True).load_state_dict(torch.load(out / "best_surv_model.pth"), strict=True)
    # the NIfTI twin trains on the same batches bit for bit, and two runs of one tree print the same line: so do the twins
    nifti_out = tmp_path / "nifti_run"
    nifti_out.mkdir()
    assert _epoch_line(log) == _epoch_line(_main([*train, *loc(ntree)], nifti_out))
    log = _main(["--inference", "--images", "--preop", "--survival", "--transforms", "--scan_space", "--weights", str(out / "best_surv_model.pth"),
                 *loc(tree)], out)
    assert "All C-indexes" in log
    val_uids = [int(l) for l in open(tree["val_uids"]).read().split()]
    assert len(val_uids) == 2
    index = {uid: i for i, uid in enumerate(ntree["uids"])}
    for uid in val_uids:
        d = out / "attention_maps" / f"_patient_{uid}"
        assert R.read_nifti_file(d / "t1image.nii.gz")["data"].any()
        for mod in ("t1", "t2"):
            series = dicom.read_series(os.path.join(tree["image_loc"], mod, f"SYN-{index[uid]:04d}-{mod}-a", "image"), header_only=True)
            for k in range(2):
                h = R.read_nifti_file(d / f"att_map_class{k}_on_{mod}.nii.gz")
                assert h["dim"][:4] == (3, *series.shape) and h["datatype"] == 16                # (Columns, Rows, slices)
                assert h["sform_code"] == 2 and np.array_equal(h["srow"], series.affine[:3].astype(np.float32)) and not np.array_equal(h["srow"], np.eye(4)[:3])
                assert np.isfinite(h["data"]).all() and h["data"].max() <= 1.0 and h["data"].min() >= 0.0
