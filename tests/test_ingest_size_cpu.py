"""`not gpu` tests of the chosen volume size S (1..128, default 64): the size-S restatements of tests/_ingest_sized_ref.py reproduce the
64^3 ones bit for bit, `Parser.imageSize`, `transforms.pipelines`, the header's two `_sized` entry points and their refusal of an S out
of range before any launch, and what `main.py --image_size` refuses and sets before it touches the GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from mmnn_sts_amd import transforms as T
from mmnn_sts_amd.data import ingest
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from mmnn_sts_amd.parser.parser import Parser
from tests import _ingest_ref as R
from tests import _ingest_sized_ref as Z
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


# ---- the restatements --------------------------------------------------------------------------------------------------------------
def test_sized_restatements_at_64_are_the_existing_ones_bit_for_bit():
    rng = np.random.default_rng(1)
    shape = (41, 70, 13)
    scan = R.random_scan(rng, shape, 4)
    mask = R.box_mask(shape, (3, 5, 1), (36, 69, 12), holes=((7, 8), (20,), (4,)))
    for ss, m in (((0.5, 3.0), mask), ((1.0, 0.0), np.zeros(shape, dtype=np.uint8))):
        a, b = R.ingest_ref(scan, m, ss), Z.ingest_ref(scan, m, 64, ss)
        assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and b[0].dtype == np.float64
    keep = S.keep_flags(scan, mask)
    maps = 0.25 + 0.75 * rng.random((2, 64, 64, 64))
    assert np.array_equal(S.maps_to_scan_ref(maps, keep), Z.maps_to_scan_ref(maps, keep))
    # and another S is another result of the right shape: windows and taps follow it
    plane, ext, _ = Z.ingest_ref(scan, mask, 100, (0.5, 3.0))
    assert plane.shape == (100, 100, 100) and ext == R.ingest_ref(scan, mask, (0.5, 3.0))[1]
    assert R.area_windows(ext[0], 100)[-1][1] == ext[0] and len(R.area_windows(ext[0], 100)) == 100
    small = 0.25 + 0.75 * rng.random((1, 24, 24, 24))
    out = Z.maps_to_scan_ref(small, keep)
    assert out.shape == (1, *shape) and S.taps(5, 24)[1].max() <= 23
    want = torch.nn.functional.interpolate(torch.from_numpy(small)[None], size=ext, mode="trilinear", align_corners=False)[0, 0].numpy()
    assert np.abs(Z.upsample(small[0], ext) - want).max() <= 1e-12


# ---- Parser.imageSize ----------------------------------------------------------------------------------------------------------------
def _parser(name="densenet121", data=None):
    p = Parser(None)
    p.parseConfig()
    p.config["ImageModel"]["name"] = name
    if data is not None:
        p.config["Data"] = data
    return p


def test_image_size_defaults_flag_over_config_and_refusals():
    assert _parser().imageSize() == 64 == ingest.SIZE and ingest.MAX_SIZE == 128
    assert _parser(data={"size": 96}).imageSize() == 96
    assert _parser(data={"size": 96}).imageSize(128) == 128                       # the flag goes before the config
    assert _parser(data={"size": "no"}).imageSize(64) == 64
    for bad in (0, 129, -64, "128", 64.0, True):
        for kw in (dict(data={"size": bad}), dict(flag=bad)):
            with pytest.raises(ConfigurationError, match=r"1\.\.128"):
                _parser(data=kw.get("data")).imageSize(kw.get("flag"))
    # inside 1..128 but too small for the network: the smallest admitted extent is named
    with pytest.raises(ConfigurationError, match=r"1\.\.128.*densenet121.*\b29\b"):
        _parser().imageSize(28)
    with pytest.raises(ConfigurationError, match=r"\b13\b"):
        _parser("tinydensenet").imageSize(12)
    assert _parser().imageSize(29) == 29 and _parser("tinydensenet").imageSize(13) == 13 and _parser("r3d_18").imageSize(1) == 1


@pytest.mark.parametrize("name,blocks", [("densenet121", (6, 12, 24, 16)), ("tinydensenet", (6, 12, 4))])
def test_smallest_image_size_is_the_plans(lib, name, blocks):
    from mmnn_sts_amd import _lib
    s = _parser(name).minImageSize()
    cfg = _lib.DenseNetConfig(2, 64, 32, 4, len(blocks), (ctypes.c_int32 * 8)(*blocks, *([0] * (8 - len(blocks)))), 1e-5, 0.1, 0.2)
    p = lib.mmnn_densenet_plan_create(ctypes.byref(cfg), 2, s, s, s)
    assert p
    lib.mmnn_densenet_plan_destroy(p)
    assert not lib.mmnn_densenet_plan_create(ctypes.byref(cfg), 2, s - 1, s - 1, s - 1) and b"too small" in lib.mmnn_last_error()


# ---- transforms.pipelines ------------------------------------------------------------------------------------------------------------
def test_pipelines_64_draws_what_the_module_pipelines_draw_and_128_resizes_to_128():
    train, val = T.pipelines(64)
    assert train.stages == T.train_transforms.stages and val.stages == T.val_transforms.stages
    assert train.spatial_size == T.train_transforms.spatial_size == val.spatial_size == T.val_transforms.spatial_size == (64, 64, 64)
    assert [type(t) for t in train.transforms] == [type(t) for t in T.train_transforms.transforms]
    assert [type(t) for t in val.transforms] == [type(t) for t in T.val_transforms.transforms]
    assert train.norm == T.train_transforms.norm and val.norm == T.val_transforms.norm
    a = T.pipelines()[0].set_random_state(5).randomize(6)
    b = T.pipelines(128)[0].set_random_state(5).randomize(6)
    state = T.train_transforms._rng
    try:
        c = T.train_transforms.set_random_state(5).randomize(6)
    finally:
        T.train_transforms._rng = state
    assert a == c and a == b and any(p.fire for p in a)                          # the draws do not depend on the size
    big_train, big_val = T.pipelines(128)
    assert big_val.spatial_size == (128,) * 3 == big_train.spatial_size and big_train.stages == train.stages
    assert T.pipelines(1)[1].spatial_size == (1, 1, 1)
    for bad in (0, 129, 64.0, "64", None):
        with pytest.raises(ValueError, match=r"1\.\.128"):
            T.pipelines(bad)


def test_public_resize_still_admits_upstreams_value_only():
    for size in ((128,) * 3, 128, (96, 96, 96), (64, 64, 128)):
        with pytest.raises(ValueError):
            T.Resize(spatial_size=size)
    assert T.Resize((64, 64, 64)).spatial_size == T.Resize().spatial_size == (64, 64, 64)


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_sized_calls_and_the_library_refuses_a_size_out_of_range(lib):
    from mmnn_sts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+MMNN_INGEST_SIZE\s+64\b", code) and re.search(r"#define\s+MMNN_INGEST_MAX_SIZE\s+128\b", code)
    assert re.search(r"int\s+mmnn_ingest_volume_sized\s*\(\s*const\s+mmnn_ingest_desc\s*\*\s*d\s*,\s*int32_t\s+size\s*,", code)
    assert re.search(r"int\s+mmnn_maps_to_scan_sized\s*\(\s*const\s+mmnn_maps_to_scan_desc\s*\*\s*d\s*,\s*int32_t\s+size\s*,", code)
    assert ctypes.sizeof(_lib.IngestDesc) == 36 and ctypes.sizeof(_lib.MapsToScanDesc) == 16        # the descriptors are the ones they were
    d = _lib.IngestDesc(8, 8, 8, 4, 2, 1.0, 0.0, 1.0, 0.0)
    m = _lib.MapsToScanDesc(8, 8, 8, 1)
    for size in (0, -1, 129, 1 << 20):
        assert lib.mmnn_ingest_volume_sized(ctypes.byref(d), size, None, None, None, None, None, None) == 1
        assert "size" in _lib.last_error() and "1..128" in _lib.last_error()
        assert lib.mmnn_maps_to_scan_sized(ctypes.byref(m), size, None, None, None, None, None) == 1
        assert "size" in _lib.last_error() and "1..128" in _lib.last_error()
    for size in (1, 64, 100, 128):                                    # an admitted size goes on to the next refusal
        assert lib.mmnn_ingest_volume_sized(ctypes.byref(d), size, None, None, None, None, None, None) == 1 and "null" in _lib.last_error()
        assert lib.mmnn_maps_to_scan_sized(ctypes.byref(m), size, None, None, None, None, None) == 1 and "null" in _lib.last_error()


def test_python_layer_refuses_before_the_library(monkeypatch):
    from mmnn_sts_amd import _lib

    def touched():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", touched)
    ws = torch.zeros(4096, dtype=torch.uint8)
    for maps in (torch.zeros((1, 129, 129, 129)), torch.zeros((1, 64, 64, 100)), torch.zeros((1, 100, 64, 64)), torch.zeros((1, 0, 0, 0))):
        with pytest.raises(ValueError, match=r"1\.\.128"):
            ingest.maps_to_scan(maps, (8, 8, 8), ws)
    for plane in (torch.zeros((129, 129, 129)), torch.zeros((64, 64, 100)), torch.zeros((100, 100, 100))):      # (the last: a host tensor)
        with pytest.raises(ValueError, match=r"1\.\.128"):
            ingest.ingest_volume(None, None, plane)
    for bad in (0, 129, 64.5, "64"):
        with pytest.raises(ValueError, match=r"1\.\.128"):
            ingest.IngestCollate("cpu", size=bad)
        with pytest.raises(ValueError, match=r"1\.\.128"):
            ingest.collate_volumes([[(None, None)]], "cpu", size=bad)
    assert ingest.IngestCollate("cpu").size == 64 and ingest.IngestCollate("cpu", size=128).size == 128


def test_collate_hands_its_size_on(monkeypatch):
    seen = []

    def fake_collate(patients, device, mask_resample, mask_threshold, keep_workspaces=False, size=ingest.SIZE):
        seen.append(size)
        return torch.zeros((len(patients), 1, 2, 2, 2)), torch.ones((len(patients), 1, 3), dtype=torch.int32)

    monkeypatch.setattr(ingest, "collate_volumes", fake_collate)
    items = [(ingest.RawPatient(3, [(None, None)]), torch.zeros(2), torch.ones(2))]
    ingest.IngestCollate("cpu")(items)
    ingest.IngestCollate("cpu", size=128)(items)
    assert seen == [64, 128]


# ---- main.py --image_size --------------------------------------------------------------------------------------------------------------
def test_cli_image_size_refusals_come_before_the_gpu():
    assert cli.build_arg_parser().parse_args(["--images", "--survival"]).image_size is None
    for argv, words in ((["--images", "--survival", "--image_size", "129"], ("--image_size", "1..128")),
                        (["--images", "--survival", "--image_size", "0"], ("--image_size", "1..128")),
                        (["--images", "--survival", "--image_size", "16"], ("--image_size", "1..128", "29")),
                        (["--preop", "--survival", "--image_size", "64"], ("--image_size", "--images"))):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert all(w in str(e.value) for w in words), (argv, str(e.value))
