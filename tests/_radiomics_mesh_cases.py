"""The (scan, mask, linear part) cases of the mesh-based shape tests and the tolerance of the one fp64 output that is not compared bitwise.

Each case is a case of tests/_radiomics_cases.py (`_case`) with one more key, `L`: the 3 x 3 linear part handed to `mmnn_radiomics_mesh`
(None: the identity).  MESH_CASES takes cases of tests/_radiomics_zones_cases.py as they are (flagged ones included) and adds the
smallest shapes at which a surface mesh can go wrong:

    voxel_1x1x1     a 1 x 1 x 1 volume that is all ROI: every one of its 8 cells lies in the padding
    full_3x2x4      a 3 x 2 x 4 volume that is all ROI: every face of the solid needs the padding
    all_configs     48 x 48 x 3: configuration c = 16 j + i as a 2 x 2 x 2 block at (3 i, 3 j, 0), one empty voxel between the blocks
    row_wrap        the case of the size-zone tests: voxels consecutive in memory across a row end and across a slice end
    line_1x1x300    a 1 x 1 x 300 line: doubled coordinates up to 600 on one axis
    plate_x/y/z     a plate one voxel thick along x, y, z in a 9 x 8 x 7 volume, with different extents in its plane
    ellipsoid_24    an ellipsoid in 24 x 20 x 12: more than two pair tiles of 256 vertices, not a multiple of 256 (asserted below)
    box_v258, box_v256   boxes of 1 x 9 x 12 and 2 x 9 x 10 voxels: 258 = 256 + 2 and exactly 256 vertices.  A closed surface of voxel
                    faces has an even number of crossings along every axis, so 256 k + 1 vertices do not exist; 256 k + 2 is the nearest
    *_oblique       the ellipsoid and the three plates again under OBLIQUE: anisotropic, sheared, negative determinant

Tolerance.  SurfaceArea is sum_c cfg[c] A_c; the restatement's deviation from the mpmath (40 digits) evaluation of the same integer
normals and the same doubles of L was measured on the CPU over the unflagged cases, relative to the sum of the terms' magnitudes (all
terms are non-negative: the sum itself).  The largest: 5.99 x 2^-53 (all_configs).  The device gets 8 x that, with the project's floor of 64 * 2^-53 (8 x 5.99 = 47.9:
the floor decides).  tests/test_radiomics_mesh_cpu.py asserts that the restatement stays within MEASURED.
"""
import numpy as np

from mmnn_sts_amd.data.synth_nifti import ellipsoid_mask
from tests._radiomics_cases import _case
from tests._radiomics_zones_cases import ZONE_CASES

U = 2.0 ** -53
MEASURED = 5.99 * U
BOUND = max(8.0 * MEASURED, 64.0 * U)

OBLIQUE = np.array([[0.9, 0.1, -0.05], [-0.12, -1.1, 0.2], [0.03, 0.25, 3.0]], dtype=np.float64)
assert np.linalg.det(OBLIQUE) < 0.0
FROM_ZONES = ("ellipsoid", "single_voxel", "off_grid_x13", "mask_float32", "seven_levels", "n2", "checkerboard", "six_faces", "row_wrap",
              "lattice", "overflow", "nan_inside", "empty")
FLAGGED = ("overflow", "nan_inside", "empty")
TILE = 256                                      # vertices per pair tile in csrc/radiomics_mesh.hip


def _one_bin(shape, roi, L=None):
    return dict(_case(np.full(shape, 130, np.int16), roi.astype(np.uint8)), L=L)


def all_configs_roi():
    roi = np.zeros((48, 48, 3), bool)
    for c in range(256):
        i, j = c % 16, c // 16
        for k in range(8):
            roi[3 * i + (k & 1), 3 * j + (k >> 1 & 1), k >> 2] = bool(c >> k & 1)
    return roi


def build():
    c = {k: dict(ZONE_CASES[k], L=None) for k in FROM_ZONES}
    c["voxel_1x1x1"] = _one_bin((1, 1, 1), np.ones((1, 1, 1), bool))
    c["full_3x2x4"] = _one_bin((3, 2, 4), np.ones((3, 2, 4), bool))
    c["all_configs"] = _one_bin((48, 48, 3), all_configs_roi())
    c["line_1x1x300"] = _one_bin((1, 1, 300), np.ones((1, 1, 300), bool))
    plates = {}
    for name, sl in (("plate_x", (slice(4, 5), slice(1, 7), slice(2, 6))), ("plate_y", (slice(0, 8), slice(3, 4), slice(1, 4))),
                     ("plate_z", (slice(2, 9), slice(2, 7), slice(6, 7)))):
        roi = np.zeros((9, 8, 7), bool)
        roi[sl] = True
        plates[name] = roi
        c[name] = _one_bin((9, 8, 7), roi)
    rng = np.random.default_rng(5150)
    ell = ellipsoid_mask((24, 20, 12), rng) != 0
    c["ellipsoid_24"] = _one_bin((24, 20, 12), ell)
    for name, box in (("box_v258", (1, 9, 12)), ("box_v256", (2, 9, 10))):
        roi = np.zeros(tuple(b + 2 for b in box), bool)
        roi[1:-1, 1:-1, 1:-1] = True
        c[name] = _one_bin(roi.shape, roi)
    c["ellipsoid_24_oblique"] = _one_bin((24, 20, 12), ell, OBLIQUE)
    for name, roi in plates.items():
        c[name + "_oblique"] = _one_bin((9, 8, 7), roi, OBLIQUE)
    return c


MESH_CASES = build()
# vertex counts the pair kernel's tiling is tested at, as counted by the restatement (tests/test_radiomics_mesh_cpu.py asserts them)
VERTICES = {"box_v258": 258, "box_v256": 256, "voxel_1x1x1": 6, "full_3x2x4": 52, "line_1x1x300": 1202}

# The MLP at the widths the mesh columns bring (one modality with every class, the size zones and the mesh: 106; two such modalities
# behind the 32 clinical columns: 244): input stream per width, by the rule written beside MLP_STREAM in tests/_radiomics_texture_cases.py;
# found on the CPU: width 106 skips streams 0 and 1 (torch's own fp32 evaluation is off the fp64 one by more than the quarter bar there);
# test_radiomics_mesh_cpu.py asserts the rule.
MLP_STREAM = {106: 2, 244: 0}
