"""The (scan, mask) cases of the size-zone tests (GLSZM) and the tolerances of their fp64 features.

ZONE_CASES takes cases of tests/_radiomics_texture_cases.py as they are and adds the smallest shapes at which a labelling can go wrong:

    corner_stairs   8^3, one bin, the voxels (t, t, t): one zone of 8 (an 18- or 6-connected labelling gives 8 zones)
    row_wrap        5 x 4 x 3, one bin, two pairs of voxels that are consecutive in memory, one across a row end (x = 4 -> x = 0 of the next
                    row) and one across a slice end; no two of the four are 26-neighbours (asserted below): 4 zones of 1
    serpentine      24 x 23 x 5, one bin: the even rows of the even slices are full, each joined to the next even row by one voxel at
                    alternating ends, the even slices joined by one voxel: one zone of 899 whose ends are as far apart in memory as the volume
                    allows -- long parent chains, merges across every chunk border
    comb            17 x 9 x 3, one bin, in the slices z = 0 and z = 2: teeth along y at the even x that meet only in the last row (the
                    teeth's roots are settled before the link that joins them is seen): 2 zones of 89
    lattice         16 x 16 x 8, the even (x, y, z) only, three levels at random: 256 zones of size 1, three keys shared by many zones
    noise_ng8 / noise_ng2     20 x 18 x 10, whole volume, 8 and 2 levels at random: hundreds of zones of many sizes / two interlocked zones
    big_zone        48 x 48 x 32 constant: one zone of 73 728, a size beyond 16 bits

The kernels of csrc/radiomics_zones.hip keep both hash tables in global memory at every Ng: there is no LDS / global threshold to
straddle.  EXPECT holds, per case, (number of zones, largest zone, distinct (level, size) pairs) as counted by hand or by the CPU restatement.

Tolerances.  For every unflagged case the numpy restatement's deviation from the mpmath evaluation of the same integer tables was measured
on the CPU, per class and relative to each feature's scale (tests/_radiomics_zones_ref.py); the largest over the cases, in units of 2^-53:

    glszm_sum 2.66    glszm_entropy 2.86

The device sums in another order with another log2, so it gets 8 x that, with a floor of 64 * 2^-53 (the floor decides in both classes).
MEASURED holds the measured figures, last digit rounded up; test_radiomics_zones_cpu.py asserts that the restatement stays within them.
"""
import itertools

import numpy as np

from tests._radiomics_cases import _case
from tests._radiomics_texture_cases import TEXTURE_CASES

U = 2.0 ** -53
MEASURED = {"glszm_sum": 2.66 * U, "glszm_entropy": 2.86 * U}
BOUND = {k: max(8.0 * v, 64.0 * U) for k, v in MEASURED.items()}

FROM_TEXTURE = ("ellipsoid", "whole_volume", "whole_volume_vec4", "single_voxel", "off_grid_x13", "off_grid_x12", "mask_float32", "seven_levels",
                "n2", "n3", "n4", "global_ng240", "constant", "constant_plane_cleared", "constant_one_voxel", "checkerboard", "six_faces",
                "long_row", "run_ng300_l64", "nbhd_ng128", "nbhd_ng129", "overflow", "nan_inside", "empty")
ROW_WRAP = ((4, 0, 0), (0, 1, 0), (4, 3, 1), (0, 0, 2))          # (x, y, z): linear indices 4, 5 and 39, 40 of the 5 x 4 x 3 volume


def _one_bin(shape, roi):
    return _case(np.full(shape, 130, np.int16), roi.astype(np.uint8))


def build():
    c = {k: TEXTURE_CASES[k] for k in FROM_TEXTURE}
    rng = np.random.default_rng(7321)
    roi = np.zeros((8, 8, 8), bool)
    roi[np.arange(8), np.arange(8), np.arange(8)] = True
    c["corner_stairs"] = _one_bin((8, 8, 8), roi)
    roi = np.zeros((5, 4, 3), bool)
    lin = [x + 5 * (y + 4 * z) for x, y, z in ROW_WRAP]
    assert lin[1] == lin[0] + 1 and lin[3] == lin[2] + 1 and ROW_WRAP[0][1] != ROW_WRAP[1][1] and ROW_WRAP[2][2] != ROW_WRAP[3][2]
    for p, q in itertools.combinations(ROW_WRAP, 2):
        assert max(abs(a - b) for a, b in zip(p, q)) > 1, (p, q)          # no two of them are 26-neighbours
    for p in ROW_WRAP:
        roi[p] = True
    c["row_wrap"] = _one_bin((5, 4, 3), roi)
    roi = np.zeros((24, 23, 5), bool)
    roi[:, 0::2, 0::2] = True
    for k, y in enumerate(range(1, 23, 2)):
        roi[23 if k % 2 == 0 else 0, y, 0::2] = True
    roi[23, 22, 1] = roi[0, 0, 3] = True
    c["serpentine"] = _one_bin((24, 23, 5), roi)
    roi = np.zeros((17, 9, 3), bool)
    roi[0::2, :8, 0::2] = True
    roi[:, 8, 0::2] = True
    c["comb"] = _one_bin((17, 9, 3), roi)
    roi = np.zeros((16, 16, 8), bool)
    roi[0::2, 0::2, 0::2] = True
    lv = rng.choice([0, 25, 50], (16, 16, 8)).astype(np.int16)
    lv[0, 0, 0], lv[2, 0, 0], lv[4, 0, 0] = 0, 25, 50
    c["lattice"] = _case(lv, roi.astype(np.uint8))
    s = (20, 18, 10)
    for ng in (8, 2):
        v = (25 * rng.integers(0, ng, s)).astype(np.int16)
        v.flat[0], v.flat[1] = 0, 25 * (ng - 1)
        c[f"noise_ng{ng}"] = _case(v, np.ones(s, np.uint8))
    c["big_zone"] = _one_bin((48, 48, 32), np.ones((48, 48, 32), bool))
    return c


ZONE_CASES = build()
FLAGGED = ("overflow", "nan_inside", "empty")
SMALL = tuple(k for k, v in ZONE_CASES.items() if v["scan"].size <= 5000)       # the flood fill in plain python runs on these
# (zones, largest zone, distinct (level, size) pairs)
EXPECT = {"constant": (1, 1170, 1), "constant_plane_cleared": (2, 585, 2), "checkerboard": (2, 585, 2), "corner_stairs": (1, 8, 1),
          "row_wrap": (4, 1, 1), "serpentine": (1, 899, 1), "comb": (2, 89, 1), "lattice": (256, 1, 3), "big_zone": (1, 73728, 1),
          "single_voxel": (1, 1, 1), "noise_ng8": (444, 351, 92), "noise_ng2": (2, 1828, 2), "run_ng300_l64": (8874, 4, 503)}

# The MLP at the widths the size-zone columns bring (one modality with all classes, two modalities of 98 behind the 32 clinical columns;
# 196 = 2 x 98 is covered by tests/test_radiomics_texture_gpu.py): input stream per width, by the rule written beside MLP_STREAM in
# tests/_radiomics_texture_cases.py.  Found on the CPU: both widths skip stream 0 (torch fp32 1.38e-5 and 6.61e-6 off the fp64 reference,
# above the quarter bar of 5e-6); test_radiomics_zones_cpu.py asserts the rule.
MLP_STREAM = {98: 1, 228: 1}
