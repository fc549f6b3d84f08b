"""`not gpu` side of occlusion sensitivity: the window grid of the numpy restatement (tests/_occlusion_ref.py), `mmnn_occlusion_window_count`
against it, the host-side refusals of the three launching calls (fake pointers, never dereferenced), the CLI flags and their rules, and
the `OcclusionSensitivity` constructor."""
import ctypes
import os

import pytest

from tests import _occlusion_ref as O


# ---- the restatement's window grid ------------------------------------------------------------------------------------------------------
def test_every_voxel_is_covered_by_a_contiguous_window_range():
    for L in range(1, 20):
        for w in range(1, L + 1):
            for s in range(1, w + 1):
                origins = O.axis_windows(L, w, s)
                assert len(origins) == -(-(L - w) // s) + 1 and origins[0] == 0 and origins[-1] == L - w
                assert all(0 <= o and o + w <= L for o in origins)
                for p, cover in enumerate(O.axis_cover(L, w, s)):
                    assert cover, (L, w, s, p)
                    assert cover == list(range(cover[0], cover[-1] + 1)), (L, w, s, p, cover)


def test_a_stride_above_the_window_is_no_grid():
    with pytest.raises(AssertionError):
        O.axis_windows(10, 2, 3)


# ---- the C-ABI without a GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def _desc(c=2, d=8, h=8, w=16, win=(4, 4, 8), stride=(4, 2, 4)):
    from mmnn_sts_amd import _lib
    return _lib.OcclusionDesc(c, d, h, w, (ctypes.c_int32 * 3)(*O.triple(win)), (ctypes.c_int32 * 3)(*O.triple(stride)))


@pytest.mark.parametrize("shape,win,stride", [
    ((9, 10, 13), (4, 3, 5), (2, 3, 4)), ((8, 8, 16), (4, 4, 8), (4, 2, 4)), ((64, 64, 64), 16, 8), ((32, 32, 32), 16, 8),
    ((5, 6, 7), (5, 6, 7), (1, 2, 3)),           # w = L: one window
    ((6, 9, 12), (2, 3, 4), (2, 3, 4)),          # s = w: a tiling
    ((3, 4, 5), 1, 1),                           # w = 1: one window per voxel
    ((7, 7, 7), (3, 3, 3), (3, 3, 3)),           # s = w with a clamped last window
])
def test_window_count_equals_the_restatement(lib, shape, win, stride):
    n = (ctypes.c_int32 * 3)()
    d = _desc(1, *shape, win=win, stride=stride)
    _, counts, wn = O.grid(shape, win, stride)
    assert lib.mmnn_occlusion_window_count(ctypes.byref(d), n) == wn and list(n) == counts
    assert lib.mmnn_occlusion_window_count(ctypes.byref(d), None) == wn


def test_the_defaults_give_343_windows(lib):
    assert lib.mmnn_occlusion_window_count(ctypes.byref(_desc(2, 64, 64, 64, 16, 8)), None) == 343 == O.grid((64, 64, 64), 16, 8)[2]


X, F, OUT, BASE, SC, WS = 0x7F0000100000, 0x7F0000200000, 0x7F0000900000, 0x7F0000300000, 0x7F0000400000, 0x7F0000500000
_BAD_DESC = {
    "zero extent": (dict(h=0), "non-positive extent"), "negative channels": (dict(c=-1), "non-positive extent"),
    "window above the extent": (dict(win=(4, 9, 8)), r"win\[1\] = 9 outside 1\.\.8"), "window zero": (dict(win=(0, 4, 8)), r"win\[0\] = 0 outside"),
    "stride above the window": (dict(stride=(4, 2, 9)), r"stride\[2\] = 9 outside 1\.\.8"), "stride zero": (dict(stride=(4, 0, 4)), r"stride\[1\] = 0 outside"),
    "2^31 elements": (dict(c=8, d=1024, h=1024, w=256, win=4, stride=4), r"2\^31 elements"),
}


@pytest.mark.parametrize("name", sorted(_BAD_DESC))
def test_a_bad_descriptor_is_refused_by_all_four_calls(lib, name):
    from mmnn_sts_amd import _lib
    fields, reason = _BAD_DESC[name]
    d = _desc(**fields)
    assert lib.mmnn_occlusion_window_count(ctypes.byref(d), None) == -1
    with pytest.raises(ValueError, match=reason):
        _lib.check(1, "mmnn_occlusion_window_count")
    assert lib.mmnn_occlude_windows(ctypes.byref(d), X, F, 0, 1, OUT, None) == 1
    with pytest.raises(ValueError, match="occlude_windows: .*" + reason):
        _lib.check(1, "mmnn_occlude_windows")
    assert lib.mmnn_occlusion_map(ctypes.byref(d), 2, BASE, SC, OUT, None) == 1
    with pytest.raises(ValueError, match="occlusion_map: .*" + reason):
        _lib.check(1, "mmnn_occlusion_map")


# Wn of the good descriptor: 2 * 3 * 3 = 18; one sample holds 2 * 8 * 8 * 16 floats = 8 KiB
_BAD_OCCLUDE = {
    "null x": (dict(x=0), "null"), "null fill": (dict(fill=0), "null"), "null out": (dict(out=0), "null"),
    "first negative": (dict(first=-1), r"first = -1 outside 0\.\.17"), "first is Wn": (dict(first=18), r"first = 18 outside 0\.\.17"),
    "count zero": (dict(count=0), "count = 0"), "count negative": (dict(count=-2), "count = -2"),
    "2^31 elements with count": (dict(count=1 << 20), r"count = 1048576 .*2\^31 elements"),
    "x misaligned": (dict(x=X + 2), "not aligned to 4"), "fill misaligned": (dict(fill=F + 1), "not aligned to 4"),
    "out misaligned": (dict(out=OUT + 3), "not aligned to 4"),
    "out inside x": (dict(out=X + 4096), "x and out overlap"), "x inside out": (dict(x=OUT + 8192, count=3), "x and out overlap"),
}


@pytest.mark.parametrize("name", sorted(_BAD_OCCLUDE))
def test_occlude_windows_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    fields, reason = _BAD_OCCLUDE[name]
    a = dict(dict(x=X, fill=F, first=0, count=2, out=OUT), **fields)
    assert lib.mmnn_occlude_windows(ctypes.byref(_desc()), a["x"] or None, a["fill"] or None, a["first"], a["count"], a["out"] or None, None) == 1
    with pytest.raises(ValueError, match="occlude_windows: .*" + reason):
        _lib.check(1, "mmnn_occlude_windows")


_BAD_MAP = {
    "null base": (dict(base=0), "null"), "null scores": (dict(scores=0), "null"), "null out": (dict(out=0), "null"),
    "k zero": (dict(k=0), r"k = 0 outside 1\.\.16"), "k seventeen": (dict(k=17), r"k = 17 outside 1\.\.16"),
    "base misaligned": (dict(base=BASE + 2), "not aligned to 4"), "scores misaligned": (dict(scores=SC + 1), "not aligned to 4"),
    "out misaligned": (dict(out=OUT + 2), "not aligned to 4"),
    "scores inside out": (dict(scores=OUT + 64), "overlap"), "base inside out": (dict(base=OUT + 4096), "overlap"),
}


@pytest.mark.parametrize("name", sorted(_BAD_MAP))
def test_occlusion_map_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    fields, reason = _BAD_MAP[name]
    a = dict(dict(k=2, base=BASE, scores=SC, out=OUT), **fields)
    assert lib.mmnn_occlusion_map(ctypes.byref(_desc()), a["k"], a["base"] or None, a["scores"] or None, a["out"] or None, None) == 1
    with pytest.raises(ValueError, match="occlusion_map: .*" + reason):
        _lib.check(1, "mmnn_occlusion_map")


def test_null_descriptors_are_refused(lib):
    from mmnn_sts_amd import _lib
    assert lib.mmnn_occlusion_window_count(None, None) == -1
    assert lib.mmnn_occlude_windows(None, X, F, 0, 1, OUT, None) == 1
    assert lib.mmnn_occlusion_map(None, 2, BASE, SC, OUT, None) == 1
    with pytest.raises(ValueError, match="null descriptor"):
        _lib.check(1, "mmnn_occlusion_map")


_BAD_MEANS = {
    "null x": (dict(x=0), "null"), "null out": (dict(out=0), "null"), "null workspace": (dict(ws=0), "null"),
    "zero channels": (dict(c=0), "c = 0 outside"), "zero elements": (dict(n=0), "non-positive extent n = 0"),
    "negative elements": (dict(n=-5), "non-positive extent n = -5"), "x misaligned": (dict(x=X + 2), "not aligned to 4"),
    "out misaligned": (dict(out=OUT + 1), "not aligned to 4"), "workspace misaligned": (dict(ws=WS + 4), "workspace not aligned to 8"),
}


@pytest.mark.parametrize("name", sorted(_BAD_MEANS))
def test_channel_means_refuses_before_launching(lib, name):
    from mmnn_sts_amd import _lib
    fields, reason = _BAD_MEANS[name]
    a = dict(dict(x=X, c=2, n=1170, out=OUT, ws=WS), **fields)
    assert lib.mmnn_channel_means(a["x"] or None, a["c"], a["n"], a["out"] or None, a["ws"] or None, None) == 1
    with pytest.raises(ValueError, match="channel_means: .*" + reason):
        _lib.check(1, "mmnn_channel_means")


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
def _main():
    import main
    return main


def test_the_new_flags_parse():
    ap = _main().build_arg_parser()
    a = ap.parse_args([])
    assert (a.occlusion, a.occlusion_window, a.occlusion_stride, a.occlusion_batch) == (False, 16, 8, 8)
    a = ap.parse_args(["--occlusion", "--occlusion_window", "12", "--occlusion_stride", "6", "--occlusion_batch", "4"])
    assert (a.occlusion, a.occlusion_window, a.occlusion_stride, a.occlusion_batch) == (True, 12, 6, 4)


@pytest.mark.parametrize("argv,names", [
    (["--survival", "--images", "--occlusion"], ["--inference"]),
    (["--survival", "--inference", "--preop", "--occlusion"], ["--images"]),
    (["--survival", "--occlusion"], ["--inference", "--images"]),
    (["--survival", "--inference", "--images", "--bootstrap", "--occlusion"], ["--bootstrap"]),
    (["--survival", "--inference", "--images", "--occlusion", "--occlusion_window", "4", "--occlusion_stride", "5"], ["--occlusion_stride", "--occlusion_window"]),
    (["--survival", "--inference", "--images", "--occlusion", "--occlusion_batch", "0"], ["--occlusion_batch"]),
])
def test_occlusion_names_what_is_missing(argv, names):
    with pytest.raises(SystemExit) as e:
        _main().main(argv)
    assert str(e.value).startswith("--occlusion") and all(n in str(e.value) for n in names)


def test_scan_space_still_needs_gradcam_on():
    with pytest.raises(SystemExit, match="--scan_space lays the Grad-CAM attention maps"):
        _main().main(["--survival", "--inference", "--images", "--no_gradcam", "--occlusion", "--scan_space"])


# ---- the constructor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,reason", [
    (dict(window=0), "window"), (dict(window=(4, 4)), "window"), (dict(window=2.5), "window"), (dict(window=True), "window"),
    (dict(stride=0), "stride"), (dict(stride=(1, 2, -3)), "stride"), (dict(window=4, stride=5), "stride 5 exceeds window 4"),
    (dict(window=(8, 8, 2), stride=(4, 4, 3)), "stride 3 exceeds window 2 on axis 2"),
    (dict(batch=0), "batch"), (dict(batch=1.5), "batch"), (dict(batch=None), "batch"),
    (dict(fill="median"), "fill"), (dict(fill=float("nan")), "fill"), (dict(fill=float("inf")), "fill"), (dict(fill=None), "fill"),
])
def test_the_constructor_rejects_bad_settings(kw, reason):
    import torch
    from mmnn_sts_amd.utils.utils import OcclusionSensitivity
    with pytest.raises(ValueError, match=reason):
        OcclusionSensitivity(torch.nn.Identity(), **kw)


def test_the_constructor_keeps_good_settings():
    import torch
    from mmnn_sts_amd.utils.utils import OcclusionSensitivity, add_occlusion
    occ = OcclusionSensitivity(torch.nn.Identity(), window=(4, 6, 8), stride=2, batch=3, fill=0)
    assert (occ.window, occ.stride, occ.batch, occ.fill, occ.multimodal) == ((4, 6, 8), (2, 2, 2), 3, 0.0, False)
    twin = add_occlusion(torch.nn.Identity(), multimodal=True, window=8, stride=8)
    assert isinstance(twin, OcclusionSensitivity) and twin.multimodal and twin.fill == "mean" and twin.batch == 8
