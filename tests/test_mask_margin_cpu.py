"""The mask margin without a device: the host queries of `mmnn_mask_margin` and their refusals, the header, the numpy restatement
(tests/_mask_margin_ref.py: brute force against the separable form, and against scipy's EDT), the shell columns, and the config / flag
parsing of `Data: mask_margin_mm` and `Radiomics: shell_mm`."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import ingest
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
from mmnn_sts_amd.parser.parser import Parser
from tests import _mask_margin_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACINGS = [(1.0, 1.0, 1.0), (0.8, 0.8, 5.0), (0.4, 0.4, 3.3)]
RADII = [0.5, 5.0, 7.3, 30.0]
EDT_SEEDS = range(12)


@pytest.mark.parametrize("spacing,radius", list(itertools.product(SPACINGS, RADII)))
def test_reach_against_the_restatement(spacing, radius):
    want = M.reach(spacing, radius)
    assert ingest.margin_reach(spacing, radius) == want
    r2 = np.float64(radius) * np.float64(radius)
    for k, s in zip(want, spacing):
        assert M.term(k, s) <= r2 < M.term(k + 1, s)


def test_reach_of_zero_on_one_axis_and_on_all():
    assert ingest.margin_reach((0.8, 0.8, 5.0), 4.0) == (5, 5, 0)
    assert ingest.margin_reach((0.8, 0.8, 5.0), 5.0) == (6, 6, 1)            # 5 mm is exactly one slice away: on the sphere, in
    assert ingest.margin_reach((1.0, 1.0, 1.0), 0.5) == (0, 0, 0)
    assert ingest.margin_reach((0.4, 0.4, 3.3), 30.0) == (75, 75, 9)


def test_host_queries_refuse():
    lib = _lib.lib()
    reach = (ctypes.c_int32 * 3)(7, 7, 7)
    ok = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    for spacing, radius in [((0.0, 1, 1), 5.0), ((1, -1.0, 1), 5.0), ((1, 1, float("nan")), 5.0), ((1, float("inf"), 1), 5.0),
                            ((1, 1, 1), 0.0), ((1, 1, 1), -2.0), ((1, 1, 1), float("nan")), ((1, 1, 1), float("inf")),
                            ((0.4, 0.4, 3.3), 0.4 * (_lib.MARGIN_MAX_REACH + 1))]:
        assert lib.mmnn_mask_margin_reach((ctypes.c_double * 3)(*spacing), radius, reach) == 1, (spacing, radius)
        assert "mask_margin" in _lib.last_error()
        assert list(reach) == [7, 7, 7]                                      # a refused query writes nothing
    assert lib.mmnn_mask_margin_reach(None, 5.0, reach) == 1 and lib.mmnn_mask_margin_reach(ok, 5.0, None) == 1
    # the cap itself is admitted, one more voxel is not
    assert ingest.margin_reach((1.0, 1.0, 1.0), float(_lib.MARGIN_MAX_REACH)) == (_lib.MARGIN_MAX_REACH,) * 3
    with pytest.raises(ValueError, match="reaches more than"):
        ingest.margin_reach((1.0, 1.0, 1.0), float(_lib.MARGIN_MAX_REACH + 1))


def test_workspace_bytes_without_gpu():
    up = lambda v: (v + 255) // 256 * 256
    for x, y, z in [(1, 1, 1), (37, 21, 9), (512, 512, 48)]:
        n = x * y * z
        assert ingest.mask_margin_workspace_bytes(x, y, z) == up(n) + up(8 * n)
    lib = _lib.lib()
    for bad in [(0, 4, 4), (4, -1, 4), (4, 4, 0), (2048, 2048, 512)]:
        assert lib.mmnn_mask_margin_workspace_bytes(*bad) == -1
        with pytest.raises(ValueError, match="mask_margin"):
            ingest.mask_margin_workspace_bytes(*bad)


def test_call_refuses_before_any_launch_without_gpu():
    """Null pointers, extents, type code, spacing, radius, mode, reach and overlap are all refused on the host: no device is touched."""
    lib = _lib.lib()
    mask = np.zeros(64, dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    ws = np.zeros(4096 + 256, dtype=np.uint8)
    wsp = (ws.ctypes.data + 255) // 256 * 256

    def desc(x=4, y=4, z=4, code=2, spacing=(1.0, 1.0, 1.0), radius=2.0, mode=_lib.MARGIN_DILATE):
        return _lib.MaskMarginDesc(x, y, z, code, 1.0, 0.0, (ctypes.c_double * 3)(*spacing), radius, mode)

    def refused(d, m=mask.ctypes.data, o=out.ctypes.data, w=wsp, what="mask_margin"):
        assert lib.mmnn_mask_margin(None if d is None else ctypes.byref(d), m, o, None, w, None) == 1
        assert what in _lib.last_error(), _lib.last_error()

    refused(None, what="null descriptor")
    refused(desc(), m=None, what="null")
    refused(desc(), o=None, what="null")
    refused(desc(), w=None, what="null")
    refused(desc(x=0), what="non-positive extent")
    refused(desc(z=-3), what="non-positive extent")
    refused(desc(x=2048, y=2048, z=512), what="2^31")
    refused(desc(code=3), what="datatype code")
    refused(desc(spacing=(1.0, 0.0, 1.0)), what="spacing[1]")
    refused(desc(spacing=(1.0, 1.0, float("nan"))), what="spacing[2]")
    refused(desc(radius=0.0), what="radius")
    refused(desc(radius=float("inf")), what="radius")
    refused(desc(mode=2), what="mode")
    refused(desc(mode=-1), what="mode")
    refused(desc(radius=_lib.MARGIN_MAX_REACH + 1.0), what="reaches more than")
    refused(desc(), o=mask.ctypes.data, what="overlap")
    refused(desc(), o=mask.ctypes.data + 63, what="overlap")
    wide = np.zeros(64, dtype=np.float64)
    refused(desc(code=64), m=wide.ctypes.data, o=wide.ctypes.data + 64 * 8 - 1, what="overlap")
    assert not out.any() and not ws.any()


def test_header_states_the_struct_and_the_cap():
    hdr = open(os.path.join(ROOT, "include", "mmnn_sts.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*mmnn_mask_margin_desc;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        assert ctype in ("int32_t", "float", "double"), decl
        fields += [(ctype, n.strip()) for n in names.split(",")]
    assert fields == [("int32_t", "x"), ("int32_t", "y"), ("int32_t", "z"), ("int32_t", "mask_type"), ("double", "mask_slope"),
                      ("double", "mask_inter"), ("double", "spacing[3]"), ("double", "radius"), ("int32_t", "mode")]
    ctypes_of = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    for (ctype, name), (field, t) in zip(fields, _lib.MaskMarginDesc._fields_):
        assert name.split("[")[0] == field
        assert t is ctypes_of[ctype] or (issubclass(t, ctypes.Array) and t._type_ is ctypes_of[ctype] and f"[{t._length_}]" in name)
    assert ctypes.sizeof(_lib.MaskMarginDesc) == 16 + 16 + 24 + 8 + 8
    macros = dict(re.findall(r"^#define\s+(MMNN_MARGIN_\w+)\s+(\d+)", hdr, flags=re.M))
    assert int(macros["MMNN_MARGIN_MAX_REACH"]) == _lib.MARGIN_MAX_REACH >= 75
    assert (int(macros["MMNN_MARGIN_DILATE"]), int(macros["MMNN_MARGIN_SHELL"])) == (_lib.MARGIN_DILATE, _lib.MARGIN_SHELL) == (0, 1)
    # the widest staged tile (csrc/mask_margin.hip: (64 + 2 reach) rows of 20 fp64 and 2 reach + 8 terms) inside the 64 KiB of a launch
    assert ((64 + 2 * _lib.MARGIN_MAX_REACH) * 20 + 2 * _lib.MARGIN_MAX_REACH + 8) * 8 <= 64 * 1024 and _lib.MARGIN_MAX_REACH < 255
    sig = _lib._signatures()
    assert all(k in sig for k in ("mmnn_mask_margin", "mmnn_mask_margin_reach", "mmnn_mask_margin_workspace_bytes"))


def _small_cases():
    rng = np.random.default_rng(20)
    for seed in range(12):
        shape = tuple(int(v) for v in rng.integers(1, 12, 3))
        spacing = [(1.0, 1.0, 1.0), tuple(rng.uniform(0.3, 4.0, 3)), (0.8, 0.8, 5.0)][seed % 3]
        yield seed, M.random_mask(shape, rng.uniform(0.02, 0.3), seed) > 0, spacing


def test_separable_form_is_the_brute_force_minimum_bit_for_bit():
    for seed, flags, spacing in _small_cases():
        want = M.brute(flags, spacing)
        assert np.array_equal(M.separable(flags, spacing), want), seed
        for radius in (0.9 * min(spacing), 2.5, 7.3):
            r = M.reach(spacing, radius)
            for mode in ("dilate", "shell"):
                a, b = M.threshold(M.separable(flags, spacing, r), radius, mode), M.threshold(want, radius, mode)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (seed, radius, mode)
    empty = np.zeros((3, 4, 2), dtype=bool)
    assert np.isinf(M.brute(empty, (1, 1, 1))).all() and np.isinf(M.separable(empty, (1, 1, 1))).all()


def test_set_voxel_rule():
    raw = np.array([[[0, 1, -2]]], dtype=np.int16)
    assert M.set_voxels(raw).tolist() == [[[False, True, True]]]
    assert M.set_voxels(raw, 2.0, 4.0).tolist() == [[[True, True, False]]]              # a raw 0 becomes 4, a raw -2 becomes 0
    for off in (0.0, float("nan"), float("inf")):
        assert M.set_voxels(raw, off, 4.0).tolist() == [[[False, True, True]]]          # no scaling
    assert M.set_voxels(np.array([[[np.nan, 0.0]]])).tolist() == [[[True, False]]]


def test_restatement_against_scipy_edt():
    """Squared distances against scipy.ndimage.distance_transform_edt(sampling=spacing)^2 within 8 * 2^-53 relative (scipy returns the
    rounded root, squaring it back costs about two roundings).  Worst seen on these 12 seeds: 2.0 * 2^-53.  The thresholded sets are
    identical where no scipy distance lies within 1e-9 relative of R2, which is asserted for every seed."""
    from scipy import ndimage
    rng = np.random.default_rng(7)
    worst = 0.0
    for seed in EDT_SEEDS:
        shape = tuple(int(v) for v in rng.integers(5, 20, 3))
        spacing = [(1.0, 1.0, 1.0), tuple(float(v) for v in rng.uniform(0.3, 4.0, 3)), (0.8, 0.8, 5.0)][seed % 3]
        flags = M.random_mask(shape, 0.03, 100 + seed) > 0
        flags[tuple(int(v) // 2 for v in shape)] = True
        D = M.separable(flags, spacing)
        edt = ndimage.distance_transform_edt(~flags, sampling=spacing)
        sq = edt * edt
        rel = np.abs(D - sq) / np.where(sq > 0.0, sq, 1.0)
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 8 * 2.0 ** -53, (seed, rel.max() * 2.0 ** 53)
        assert np.array_equal(D == 0.0, edt == 0.0)
        radius = float(rng.uniform(1.5, 6.0))
        r2 = radius * radius
        assert (np.abs(sq - r2) > 1e-9 * r2).all(), (seed, "a scipy distance lies on the threshold: choose another seed")
        for mode in ("dilate", "shell"):
            got = M.threshold(D, radius, mode)[0]
            want = (edt <= radius) & ((edt > 0.0) if mode == "shell" else True)
            assert np.array_equal(got, want.astype(np.uint8)), (seed, mode)
    print("worst relative deviation of D from scipy's EDT^2, in units of 2^-53:", worst * 2.0 ** 53)


def test_feature_names_with_shells():
    base = radiomics.feature_names()
    assert radiomics.feature_names(shell_mm=()) == base and radiomics.feature_names(shell_mm=None) == base
    one = radiomics.feature_names(shell_mm=[5])
    assert one[:len(base)] == base and len(one) == len(base) + 18 + 23
    assert one[len(base)] == "shell-5-0-mm_firstorder_Energy" and one[-1] == "shell-5-0-mm_glcm_SumSquares"
    assert not [n for n in one[len(base):] if "_shape_" in n]
    assert radiomics.shell_image_type(7.5) == "shell-7-5-mm" and radiomics.shell_widths("10, 5,5") == (5.0, 10.0)
    full = radiomics.feature_names("all", True, True, (1.0,), (10, 5))
    head = radiomics.feature_names("all", True, True, (1.0,))
    assert full[:len(head)] == head                                                   # behind every original_* and log-* column
    per = 18 + 23 + 16 + 14 + 5 + 16
    assert len(full) == len(head) + 2 * per
    assert full[len(head)].startswith("shell-5-0-mm_") and full[len(head) + per].startswith("shell-10-0-mm_")
    assert [n.split("_", 1)[1] for n in full[len(head):len(head) + per]] == [n.split("_", 1)[1] for n in head if n.startswith("log-sigma-1-0-mm-3D_")]
    for bad in ([0], [-1.0], ["x"], [float("inf")], [True], {"a": 1}):
        with pytest.raises(ConfigurationError):
            radiomics.shell_widths(bad)


def _parser(tmp_path, text):
    import yaml
    base = Parser(None)
    base.parseConfig()
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump({**base.config, **yaml.safe_load(text)}))
    p = Parser(str(path))
    p.parseConfig()
    return p


def test_config_and_flag_parsing(tmp_path):
    p = _parser(tmp_path, "Data:\n  mask_margin_mm: 7.5\nRadiomics:\n  shell_mm: [10, 5]\n")
    assert p.maskMargin() == 7.5 and p.maskMargin(3.0) == 3.0
    assert p.radiomicsShell() == (5.0, 10.0) and p.radiomicsShell("2.5") == (2.5,)
    q = _parser(tmp_path, "Data:\n  size: 64\n")
    assert q.maskMargin() is None and q.radiomicsShell() == ()
    for text in ("Data:\n  mask_margin_mm: 0\n", "Data:\n  mask_margin_mm: -3\n", "Data:\n  mask_margin_mm: wide\n", "Data:\n  mask_margin_mm: true\n",
                 "Data:\n  mask_margin_mm: .inf\n"):
        with pytest.raises(ConfigurationError, match="mask_margin_mm"):
            _parser(tmp_path, text).maskMargin()
    with pytest.raises(ConfigurationError, match="--mask_margin_mm"):
        q.maskMargin(-1.0)
    for text in ("Radiomics:\n  shell_mm: [0]\n", "Radiomics:\n  shell_mm: [5, no]\n", "Radiomics:\n  shell_mm: '5,10'\n", "Radiomics:\n  shell_mm: {a: 1}\n"):
        with pytest.raises(ConfigurationError, match="shell"):
            _parser(tmp_path, text).radiomicsShell()
    assert ingest.IngestCollate("cpu").mask_margin_mm is None and ingest.IngestCollate("cpu", mask_margin_mm=4).mask_margin_mm == 4.0
    with pytest.raises(ConfigurationError):
        ingest.IngestCollate("cpu", mask_margin_mm=0.0)
    a = radiomics.build_arg_parser().parse_args(["--image_loc", "x", "--key_loc", "k", "--out", "o", "--shell_mm", "5,10"])
    assert a.shell_mm == "5,10"


def test_main_refuses_the_flags_where_they_have_no_meaning():
    import main
    a = main.build_arg_parser().parse_args(["--images", "--classification", "--mask_margin_mm", "5", "--shell_mm", "5,10"])
    assert a.mask_margin_mm == 5.0 and a.shell_mm == "5,10"
    with pytest.raises(SystemExit, match="needs --image_loc"):
        main.main(["--images", "--classification", "--mask_margin_mm", "5"])
    with pytest.raises(SystemExit, match="mask_margin_mm"):
        main.main(["--images", "--classification", "--mask_margin_mm", "-5"])
    with pytest.raises(SystemExit, match="needs --radiomics"):
        main.main(["--images", "--classification", "--shell_mm", "5"])


def test_python_refuses_a_radius_below_every_spacing():
    vol = ingest.DeviceVolume(None, (4, 4, 4), 2)
    with pytest.raises(ValueError, match=r"0\.8, 0\.8, 5\.0 mm"):
        ingest.mask_margin(vol, (0.8, 0.8, 5.0), 0.5)
    with pytest.raises(ValueError, match="mode"):
        ingest.mask_margin(vol, (1, 1, 1), 5.0, mode="erode")
