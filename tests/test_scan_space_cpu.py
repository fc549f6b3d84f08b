"""`not gpu` tests of the scan-space attention maps' host side: the numpy restatement of the `mmnn_maps_to_scan` contract
(tests/_scan_space_ref.py) against torch's fp64 CPU `interpolate`, the workspace query (pure host arithmetic), the refusals of
`ingest.maps_to_scan` and of the library before any launch, `main.py --scan_space` outside its one valid combination, and the opt-in
retention of the ingest workspaces by the collate function."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from mmnn_sts_amd.data import ingest
from tests import _scan_space_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import main as cli  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [(1, 1, 1), (1, 64, 200), (37, 63, 65), (150, 9, 2), (64, 64, 64)])
def test_restatement_equals_torch_trilinear_fp64(ext):
    rng = np.random.default_rng(sum(ext))
    vol = 0.25 + 0.75 * rng.random((64, 64, 64))
    want = torch.nn.functional.interpolate(torch.from_numpy(vol)[None, None], size=ext, mode="trilinear", align_corners=False)[0, 0].numpy()
    got = S.upsample(vol, ext)
    err = float(np.abs(got - want).max())
    print(f"extents {ext}: max |restatement - torch fp64 interpolate| {err:.3e}")
    assert got.shape == ext and got.dtype == np.float64
    assert err <= 1e-12
    if ext == (64, 64, 64):
        assert np.array_equal(got, vol)                              # every coordinate an integer, every weight 0


def test_restatement_taps_and_scatter():
    i0, i1, w = S.taps(1)
    assert (i0[0], i1[0], w[0]) == (31, 32, 0.5)                         # one kept slice sits between the two central map entries
    i0, i1, w = S.taps(200)
    assert i0.min() == 0 and i1.max() == 63 and (w >= 0).all() and (w < 1).all() and (np.diff(i0) >= 0).all() and (i1 - i0 <= 1).all()
    keep = [np.array([0, 1, 1, 0, 1], bool), np.array([1, 0, 1], bool), np.array([0, 1], bool)]
    maps = 0.25 + 0.75 * np.random.default_rng(1).random((2, 64, 64, 64))
    out = S.maps_to_scan_ref(maps, keep)
    assert out.shape == (2, 5, 3, 2)
    kept = np.einsum("i,j,k->ijk", *[k.astype(int) for k in keep]).astype(bool)
    assert (out[:, kept] > 0).all() and not out[:, ~kept].any()
    assert np.array_equal(out[1][np.ix_([1, 2, 4], [0, 2], [1])], S.upsample(maps[1], (3, 2, 1)))
    assert not S.maps_to_scan_ref(maps, [keep[0], np.zeros(3, bool), keep[2]]).any()
    assert S.tolerance(maps) == 2.0 * 2.0 ** -24 * maps.max()


# ---- the library's host side ---------------------------------------------------------------------------------------------------------
def test_workspace_bytes_and_refusals_need_no_gpu(lib):
    from mmnn_sts_amd import _lib
    for ext in ((1, 1, 1), (37, 29, 11), (512, 512, 48), (2048, 1000, 1000)):
        n = lib.mmnn_maps_to_scan_workspace_bytes(*ext)
        assert n >= 16 * sum(ext) and n % 256 == 0, ext
        assert ingest.maps_to_scan_workspace_bytes(*ext) == n
    for ext in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2049, 4, 4), (2048, 1024, 1024), (1291, 1290, 1290)):
        assert lib.mmnn_maps_to_scan_workspace_bytes(*ext) == -1, ext
        with pytest.raises(ValueError):
            ingest.maps_to_scan_workspace_bytes(*ext)
    assert ctypes.sizeof(_lib.MapsToScanDesc) == 16

    def status(x=8, y=8, z=8, n=1, ptrs=(None, None, None, None)):
        d = _lib.MapsToScanDesc(x, y, z, n)
        return lib.mmnn_maps_to_scan(ctypes.byref(d), *ptrs, None), _lib.last_error()

    for kw, word in ((dict(x=0), "extent"), (dict(z=-2), "extent"), (dict(x=2049), "2048"), (dict(x=2048, y=2048, z=512), "2^31"),
                     (dict(n=0), "n_maps"), (dict(n=17), "n_maps"), (dict(), "null"), (dict(ptrs=(256, 256, None, 256)), "null")):
        st, msg = status(**kw)
        assert st == 1 and word in msg, (kw, msg)
    assert lib.mmnn_maps_to_scan(None, None, None, None, None, None) == 1


def test_maps_to_scan_refuses_before_the_library(monkeypatch):
    from mmnn_sts_amd import _lib

    def touched():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", touched)
    ws = torch.zeros(4096, dtype=torch.uint8)
    good = torch.zeros((2, 64, 64, 64))
    for maps, shape, w, word in ((torch.zeros((2, 64, 64, 63)), (8, 8, 8), ws, "maps must be (n, 64, 64, 64)"),
                                 (torch.zeros((64, 64, 64)), (8, 8, 8), ws, "maps must be (n, 64, 64, 64)"),
                                 (torch.zeros((17, 64, 64, 64)), (8, 8, 8), ws, "1..16"),
                                 (torch.zeros((0, 64, 64, 64)), (8, 8, 8), ws, "1..16"),
                                 (good.double(), (8, 8, 8), ws, "fp32"),
                                 (good.half(), (8, 8, 8), ws, "fp32"),
                                 (torch.zeros((2, 64, 64, 128))[..., ::2], (8, 8, 8), ws, "contiguous"),
                                 (good, (8, 8), ws, "scan_shape"),
                                 (good, (8, 0, 8), ws, "scan_shape"),
                                 (good, (8, 8.5, 8), ws, "scan_shape"),
                                 (good, (8, 8, 8), ws.float(), "ingest_workspace"),
                                 (good, (8, 8, 8), None, "ingest_workspace"),
                                 (good, (8, 8, 8), ws, "on the GPU")):                       # a host tensor: the wrong device
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
            ingest.maps_to_scan(maps, shape, w)


# ---- main.py --scan_space ------------------------------------------------------------------------------------------------------------
def test_scan_space_flag_outside_its_combination_exits_with_the_message(tmp_path):
    loc = ["--image_loc", str(tmp_path / "images"), "--key_loc", str(tmp_path / "key.csv"), "--data_loc", str(tmp_path / "clinical.csv")]
    for argv in (["--images", "--survival", "--scan_space"],                                  # neither --inference nor --image_loc
                 ["--inference", "--images", "--survival", "--scan_space"],                   # no --image_loc
                 ["--images", "--survival", "--scan_space", *loc],                            # no --inference
                 ["--inference", "--images", "--survival", "--scan_space", "--no_gradcam", *loc],
                 ["--inference", "--images", "--survival", "--scan_space", "--bootstrap", *loc],
                 ["--inference", "--preop", "--survival", "--scan_space"]):                    # no image model: no Grad-CAM
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        msg = str(e.value)
        assert "--scan_space" in msg and "--inference" in msg and "--image_loc" in msg and "Grad-CAM" in msg, (argv, msg)
    assert cli.build_arg_parser().parse_args(["--images", "--survival"]).scan_space is False


# ---- the collate function ------------------------------------------------------------------------------------------------------------
def test_collate_keeps_workspaces_only_when_asked(monkeypatch):
    seen = []

    def fake_collate(patients, device, mask_resample, mask_threshold, keep_workspaces=False):
        seen.append(keep_workspaces)
        n, c = len(patients), len(patients[0])
        batch, ext = torch.zeros((n, c, 2, 2, 2)), torch.ones((n, c, 3), dtype=torch.int32)
        kept = [[ingest.KeptVolume(torch.zeros(8, dtype=torch.uint8), (4, 5, 6), None) for _ in range(c)] for _ in range(n)]
        return (batch, ext, kept) if keep_workspaces else (batch, ext)

    monkeypatch.setattr(ingest, "collate_volumes", fake_collate)
    items = [(ingest.RawPatient(7 + i, [(None, None), (None, None)]), torch.zeros(2), torch.ones(2)) for i in range(3)]
    off = ingest.IngestCollate("cpu")
    assert off.keep_workspaces is False and off.last_volumes == []
    x, ev, du = off(items)
    assert seen == [False] and off.last_volumes == [] and x.shape[:2] == (3, 2) and len(off.pending) == 1      # nothing retained
    on = ingest.IngestCollate("cpu", keep_workspaces=True)
    on(items)
    on(items[:1])
    assert seen == [False, True, True]
    assert len(on.last_volumes) == 1 and len(on.last_volumes[0]) == 2 and on.last_volumes[0][0].shape == (4, 5, 6)      # the LAST batch only
