"""The (scan, mask) cases of the radiomics tests, seeded, and the tolerances of the fp64 features that are not compared bitwise.

Each case: dict(scan, mask (x, y, z arrays), bin_width, max_bins, scan_scale, mask_scale, scan_lead, mask_lead (bytes the device buffer is
moved off its 256-byte boundary)).

Tolerances.  For every case the numpy restatement's deviation from the mpmath evaluation of the same inputs was measured on the CPU,
per feature class and relative to each feature's scale (tests/_radiomics_ref.py); the largest over the cases, in units of 2^-53:

    firstorder_moment 2.84    histogram 2.37    glcm_sum 3.04    glcm_entropy 2.58

The device sums in another order and uses another log2 / exp / pow, so it gets 8 x that, with a floor of 64 * 2^-53: the floor decides
in every class (8 x 3.04 = 24.3 is the largest product).  MEASURED holds the measured figures, with the last digit rounded up;
test_radiomics_cpu.py asserts that the restatement stays within them for every case.
"""
import numpy as np

from mmnn_sts_amd.data.synth_nifti import ellipsoid_mask

U = 2.0 ** -53
MEASURED = {"firstorder_moment": 2.84 * U, "histogram": 2.37 * U, "glcm_sum": 3.04 * U, "glcm_entropy": 2.58 * U}
BOUND = {k: max(8.0 * v, 64.0 * U) for k, v in MEASURED.items()}

SCAN_DTYPES = ("uint8", "int16", "int32", "float32", "float64", "int8", "uint16", "uint32")


def _case(scan, mask, bin_width=25.0, max_bins=256, scan_scale=(1.0, 0.0), mask_scale=(1.0, 0.0), scan_lead=0, mask_lead=0):
    return dict(scan=scan, mask=mask, bin_width=bin_width, max_bins=max_bins, scan_scale=scan_scale, mask_scale=mask_scale,
                scan_lead=scan_lead, mask_lead=mask_lead)


def _typed(rng, shape, dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal(shape) * 300.0).astype(dt)
    lo, hi = max(np.iinfo(dt).min, -900), min(np.iinfo(dt).max, 900)
    return rng.integers(lo, hi + 1, shape).astype(dt)


def build():
    c = {}
    rng = np.random.default_rng(2024)
    s = (13, 10, 9)
    c["ellipsoid"] = _case(rng.integers(-200, 1800, s).astype(np.int16), ellipsoid_mask(s, rng), scan_scale=(0.25, -12.5))
    c["whole_volume"] = _case(rng.integers(0, 700, s).astype(np.int16), np.ones(s, np.uint8))
    c["whole_volume_vec4"] = _case(rng.integers(0, 700, (12, 10, 9)).astype(np.int16), np.ones((12, 10, 9), np.uint8))
    one = np.zeros(s, np.uint8)
    one[6, 4, 3] = 1
    c["single_voxel"] = _case(rng.integers(0, 700, s).astype(np.int16), one)
    c["off_grid_x13"] = _case(rng.integers(0, 700, s).astype(np.int16), ellipsoid_mask(s, rng), scan_lead=2, mask_lead=1)
    c["off_grid_x12"] = _case(rng.integers(0, 700, (12, 10, 9)).astype(np.int16), ellipsoid_mask((12, 10, 9), rng), scan_lead=6, mask_lead=3)
    for dt in SCAN_DTYPES:
        # mask values other than 0 / 1; with the mask's slope 2 and inter -6 the raw value 3 is OUTSIDE the ROI and 0 inside
        m = ellipsoid_mask((12, 11, 8), rng).astype(np.uint8) * rng.choice([3, 7, 200], (12, 11, 8)).astype(np.uint8)
        c[f"scan_{dt}"] = _case(_typed(rng, (12, 11, 8), dt), m, scan_scale=(-0.5, 100.0), mask_scale=(2.0, -6.0))
    mf = ellipsoid_mask(s, rng).astype(np.float32) * rng.choice([0.5, -2.0, 1e-30], s).astype(np.float32)
    c["mask_float32"] = _case(rng.integers(-300, 300, s).astype(np.int32), mf, scan_scale=(1.5, 0.0))
    big = (24, 20, 10)
    wide = rng.integers(0, 6000, big).astype(np.int16)
    wide[0, 0, 0], wide[1, 0, 0] = 0, 5999
    c["global_ng240"] = _case(wide, np.ones(big, np.uint8))                     # Ng = 240 > the 128 the LDS matrix holds
    c["overflow"] = _case(wide, np.ones(big, np.uint8), bin_width=5.0)           # Ng = 1200 > 256
    f = (rng.standard_normal(s) * 100.0).astype(np.float32)
    m = ellipsoid_mask(s, rng)
    inside, outside = np.argwhere(m != 0), np.argwhere(m == 0)
    f_in, f_out = f.copy(), f.copy()
    f_in[tuple(inside[len(inside) // 2])] = np.nan
    f_out[tuple(outside[len(outside) // 2])] = np.nan
    f_out[tuple(outside[0])] = np.inf
    c["nan_inside"] = _case(f_in, m)
    c["nan_outside"] = _case(f_out, m)
    c["seven_levels"] = _case(rng.choice([-40, -3, 0, 12, 77, 78, 400], s).astype(np.int16), ellipsoid_mask(s, rng))
    for n in (2, 3, 4):
        few = np.zeros(s, np.uint8)
        few[5, 4, 2:2 + n] = 1
        c[f"n{n}"] = _case(rng.integers(0, 700, s).astype(np.int16), few)
    c["empty"] = _case(rng.integers(0, 700, s).astype(np.int16), np.zeros(s, np.uint8))
    return c


CASES = build()
