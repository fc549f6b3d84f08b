"""The (scan, mask) cases of the texture tests (GLRLM, GLDM, NGTDM) and the tolerances of their fp64 features.

TEXTURE_CASES takes cases of tests/_radiomics_cases.py as they are and adds the shapes at which the texture kernels can go wrong:

    constant               one bin over the whole 13 x 10 x 9 volume: every axis run has the full extent, diagonal runs end at faces, Ngp = 1
                           (Coarseness 10^6, the other NGTDM features 0), dependence 27 in the interior
    constant_plane_cleared ... with the plane y = 4 of the mask cleared; constant_one_voxel: ... with one interior voxel of another bin
    checkerboard           two bins alternating: every axis run has length 1, no axis neighbour shares the bin
    six_faces              a 7 x 11 x 5 volume whose ROI touches all six faces (a run that wrapped a row or a slice would show)
    long_row               4100 x 1 x 2, three levels in long runs: L above the 4096 lengths whose marginal the feature kernel keeps in LDS
    run_ng256_l64 / run_ng300_l64     Ng * L = 16384 (the run-length matrix in LDS, at the limit) and 19200 (global atomics)
    nbhd_ng128 / nbhd_ng129           Ng = 128 (the neighbourhood tables in LDS, at the limit) and 129 (global atomics)
    global_ng240           of CASES: neighbourhood tables global (Ng = 240), run-length matrix in LDS (240 * 24 words)

Tolerances.  For every case the numpy restatement's deviation from the mpmath evaluation of the same integer tables was measured on the
CPU, per class and relative to each feature's scale (tests/_radiomics_texture_ref.py); the largest over the cases, in units of 2^-53:

    glrlm_sum 3.10    glrlm_entropy 2.72    gldm_sum 2.28    gldm_entropy 1.84    ngtdm 0.96

The device sums in another order with another log2, so it gets 8 x that, with a floor of 64 * 2^-53.  MEASURED holds the measured figures,
last digit rounded up (the floor decides in every class: 8 x 3.10 = 24.8 is the largest product); test_radiomics_texture_cpu.py asserts that the restatement stays within them for every case.
"""
import numpy as np

from tests._radiomics_cases import CASES, _case

U = 2.0 ** -53
MEASURED = {"glrlm_sum": 3.10 * U, "glrlm_entropy": 2.72 * U, "gldm_sum": 2.28 * U, "gldm_entropy": 1.84 * U,
            "ngtdm": 0.96 * U}
BOUND = {k: max(8.0 * v, 64.0 * U) for k, v in MEASURED.items()}

FROM_CASES = ("ellipsoid", "whole_volume", "whole_volume_vec4", "single_voxel", "off_grid_x13", "off_grid_x12", "mask_float32", "global_ng240",
              "overflow", "nan_inside", "seven_levels", "n2", "n3", "n4", "empty")
RUN_LDS_WORDS, NBHD_LDS_NG, FEATURE_LDS_L = 16384, 128, 4096      # the thresholds of csrc/radiomics_texture.hip


def _spread(rng, shape, top):
    """int16 values 0..top over `shape`, both ends present: Ng = top // 25 + 1 at bin_width 25."""
    v = rng.integers(0, top + 1, shape).astype(np.int16)
    v.flat[0], v.flat[1] = 0, top
    return v


def build():
    c = {k: CASES[k] for k in FROM_CASES}
    rng = np.random.default_rng(4048)
    s = (13, 10, 9)
    ones = np.ones(s, np.uint8)
    c["constant"] = _case(np.full(s, 130, np.int16), ones)
    cut = ones.copy()
    cut[:, 4, :] = 0
    c["constant_plane_cleared"] = _case(np.full(s, 130, np.int16), cut)
    dot = np.full(s, 130, np.int16)
    dot[6, 4, 3] = 190
    c["constant_one_voxel"] = _case(dot, ones)
    x, y, z = np.meshgrid(*[np.arange(n) for n in s], indexing="ij")
    c["checkerboard"] = _case((((x + y + z) % 2) * 25).astype(np.int16), ones)
    f = (7, 11, 5)
    roi = (rng.random(f) < 0.35).astype(np.uint8)
    roi[3, :, 2] = roi[:, 5, 2] = roi[3, 5, :] = 1       # three lines through the centre, from face to face
    roi[0, 0, :] = roi[6, 10, :] = roi[0, :, 0] = roi[6, :, 4] = 1
    c["six_faces"] = _case(rng.choice([0, 30, 60, 200], f).astype(np.int16), roi)
    row = (25 * ((np.arange(4100) // 700) % 3)).astype(np.int16)
    row[rng.integers(0, 4100, 12)] = 50
    long_row = np.stack([row, np.roll(row, 350)], axis=-1).reshape(4100, 1, 2)
    c["long_row"] = _case(long_row, np.ones((4100, 1, 2), np.uint8), max_bins=8)
    w = (64, 12, 12)
    c["run_ng256_l64"] = _case(_spread(rng, w, 6399), np.ones(w, np.uint8), max_bins=320)
    c["run_ng300_l64"] = _case(_spread(rng, w, 7499), np.ones(w, np.uint8), max_bins=320)
    c["nbhd_ng128"] = _case(_spread(rng, s, 3199), ones)
    c["nbhd_ng129"] = _case(_spread(rng, s, 3224), ones)
    return c


TEXTURE_CASES = build()
FLAGGED = ("overflow", "nan_inside", "empty")
EXPECT_NG = {"run_ng256_l64": 256, "run_ng300_l64": 300, "nbhd_ng128": 128, "nbhd_ng129": 129, "global_ng240": 240, "constant": 1, "checkerboard": 2}

# The MLP at the widths of the wider table (one modality, two, two behind the 32 clinical columns): input stream per width.  BatchNorm over
# the N = 4 rows of that test is badly conditioned for some inputs: torch's own fp32 evaluation of the fp64 reference on the CPU is
# between 1.5e-6 and 3.1e-5 off it, depending on the stream.  The stream is the first index at which (a) no pre-activation of the fp64
# reference is within 1e-4 of zero and (b) torch's fp32 evaluation is within a quarter of the bar (2e-5 / 4) of the fp64 one, so that the
# factor 4 tests/test_tail_ops_gpu.py grants another summation order stays inside the bar.  Found on the CPU: width 82 skips streams 0
# and 1 (torch fp32 1.03e-5 and 2.14e-5 off); test_radiomics_texture_cpu.py asserts the rule.
MLP_STREAM = {82: 2, 164: 0, 196: 0}
