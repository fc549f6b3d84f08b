"""The cases of the Laplacian-of-Gaussian tests, seeded.

FILTER_CASES: dict(scan (x, y, z array), spacing (mm), sigma (mm), radii (what log_taps must give), scale (slope, inter), lead (bytes the
device buffer is moved off its 256-byte boundary)).  The first five are the grids, spacings and scales the filter is specified on; the
others cover the scan types, a misaligned buffer, the x = 12 / 13 tails and the kernel's tiles.

Tiles (csrc/radiomics_filter.hip).  The x pass gives a workgroup 4 rows of 256 outputs along x; the y and z passes a tile of 16 columns
along x by 64 outputs along the filtered axis.  `tiles_xy` has x = 260 (two x tiles, the second 4 wide; 17 column tiles, the last 4 wide),
y = 66 (two tiles along y) and y * z = 198 rows (not a multiple of 4); `tiles_z` has z = 66 and x = 18.

FEATURE_CASES: dict(scan, mask, spacing, sigmas, bin_width (of the filtered images; the original image keeps 25), classes, glszm): random
int16 in [-200, 1800) under an ellipsoid mask.  Inside the mask the filtered images span 39, 11 and 10 bins of width 25, and at sigma
5 mm 14 bins of width 10 (6 of width 25); test_radiomics_log_cpu.py asserts 8 <= Ng <= 256 for each, so none can set the overflow flag
on the device.

MLP_STREAM: the input stream of the MLP test per width, by the rule of tests/_radiomics_texture_cases.py: the first index whose fp64
pre-activations stay off the ReLU branch points and whose fp32 torch evaluation is within a quarter of the bar."""
import numpy as np

from mmnn_sts_amd.data.synth_nifti import ellipsoid_mask

TILE_X, TILE_ROWS, TILE_COLUMNS, TILE_LINE = 256, 4, 16, 64
MLP_STREAM = {88: 6, 176: 4}


def _f(scan, spacing, sigma, radii, scale=(1.0, 0.0), lead=0):
    return dict(scan=scan, spacing=tuple(float(s) for s in spacing), sigma=float(sigma), radii=tuple(radii), scale=scale, lead=lead)


def _i16(rng, shape):
    return rng.integers(-200, 1800, shape).astype(np.int16)


def build_filter():
    rng = np.random.default_rng(951)
    c = {}
    c["radii_at_extent"] = _f(_i16(rng, (13, 10, 9)), (0.8, 1.1, 5.0), 3.0, (15, 11, 2))
    c["small_radii"] = _f(_i16(rng, (13, 10, 9)), (0.8, 1.1, 5.0), 1.0, (5, 4, 1))
    c["radius_above_extents"] = _f(_i16(rng, (5, 7, 3)), (1.0, 1.0, 1.0), 2.0, (8, 8, 8))
    c["larger_radii"] = _f(_i16(rng, (12, 11, 8)), (0.9, 0.9, 2.5), 5.0, (22, 22, 8))
    c["radius_64"] = _f(_i16(rng, (70, 3, 2)), (1.0, 1.0, 1.0), 16.0, (64, 64, 64))
    s = (12, 11, 8)
    c["type_uint8"] = _f(rng.integers(0, 256, s).astype(np.uint8), (0.9, 0.9, 2.5), 2.0, (9, 9, 3))
    c["type_int16_scaled"] = _f(_i16(rng, s), (0.9, 0.9, 2.5), 2.0, (9, 9, 3), scale=(-0.5, 100.0))
    c["type_float32"] = _f((rng.standard_normal(s) * 300.0).astype(np.float32), (0.9, 0.9, 2.5), 2.0, (9, 9, 3))
    c["type_float64"] = _f(rng.standard_normal(s) * 300.0, (0.9, 0.9, 2.5), 2.0, (9, 9, 3))
    c["off_boundary_x13"] = _f(_i16(rng, (13, 10, 9)), (0.8, 1.1, 5.0), 1.0, (5, 4, 1), lead=2)
    c["tail_x12"] = _f(_i16(rng, (12, 10, 9)), (0.8, 1.1, 5.0), 1.0, (5, 4, 1))
    c["tiles_xy"] = _f(_i16(rng, (260, 66, 3)), (1.0, 1.0, 1.0), 1.0, (4, 4, 4))
    c["tiles_z"] = _f(_i16(rng, (18, 3, 66)), (1.0, 1.0, 1.0), 1.0, (4, 4, 4))
    return c


def _g(rng, shape, spacing, sigmas, classes=(), glszm=False, bin_width=25.0):
    return dict(scan=_i16(rng, shape), mask=ellipsoid_mask(shape, rng), spacing=tuple(float(s) for s in spacing), sigmas=tuple(sigmas),
                bin_width=bin_width, classes=tuple(classes), glszm=glszm)


def build_features():
    rng = np.random.default_rng(952)
    return {"default_two_scales": _g(rng, (13, 10, 9), (0.8, 1.1, 5.0), (1.0, 3.0)),
            "every_class": _g(rng, (12, 11, 8), (0.9, 0.9, 2.5), (5.0,), ("glrlm", "gldm", "ngtdm"), True, bin_width=10.0),
            "isotropic_glszm": _g(rng, (13, 10, 9), (1.0, 1.0, 1.0), (2.0,), (), True)}


def affine_of(spacing):
    return np.diag(list(spacing) + [1.0])


FILTER_CASES = build_filter()
FEATURE_CASES = build_features()
