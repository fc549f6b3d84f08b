"""The cases of the normalisation and resampling tests, seeded.

NORMALIZE_CASES: dict(scan, scale (slope, inter), lead).  RESAMPLE_CASES: dict(scan, mask, spacing (of the scan, mm), to (the requested
spacing; 0 keeps an axis), out (the extents resample_grid must give), scale, lead).  The first four resample cases are the grids the
restatement is held to scipy on.

Tiles (csrc/radiomics_resample.hip).  The normalisation's sums run over min(NORM_MAX_PARTS, ceil(n / NORM_TPB)) workgroups of NORM_TPB
lanes; a workgroup makes a second trip once n > NORM_TPB * NORM_MAX_PARTS = 65536: `two_trips` has 68541 voxels, the others 2 to 5
partial sums.  A lane of the sum passes keeps NORM_BATCH loads in flight, so their batched loop runs once n > (NORM_BATCH - 1) *
NORM_MAX_PARTS * NORM_TPB = 196608; the write pass has at most NORM_WRITE_GROUPS workgroups, strides from n > NORM_WRITE_GROUPS *
NORM_TPB = 524288 and batches from n > (NORM_BATCH - 1) times that: `batched_strides` (128 x 128 x 130 = 2129920 voxels, above
NORM_BATCH * NORM_WRITE_GROUPS * NORM_TPB = 2097152 and no multiple of either batch's span) runs every batched loop and the tail behind
it.  The y / z prefilter issues the loads of LINE_BATCH samples of a line together (lines of 10, 9, 13 and 70 samples: whole batches and
tails), the staging of the x prefilter those of LINE_BATCH lines; the last gather walks Z_RUN output planes per workgroup
(`anisotropic_to_1mm` has 45: two runs and one of 13).  The x prefilter gives one wave X_LINES lines and moves chunks of X_CHUNK samples through LDS; the y / z prefilter and the
evaluation give a workgroup LINE_TPB lanes, one per line / output.  `longer_than_horizon` (x = 70) has a second chunk of 6;
`chunk_65` a second chunk of 1 (where the backward sweep starts) and `chunk_128` two whole chunks; `tiles` has x = 66, 13 * 6 = 78
lines (a fifth workgroup of 14), 66 * 6 = 396 y lines and 66 * 13 = 858 z lines (more than LINE_TPB each) and no pass's output count
is a multiple of LINE_TPB.

FEATURE_CASES: dict(scan, mask, spacing, to, classes, glszm, mesh, sigmas, log_bin_width): random int16 in [-200, 1800) under an
ellipsoid mask, normalised at scale 100 and binned at 25; test_radiomics_resample_cpu.py asserts on the restatement's output that no
flag is set, 8 <= Ng <= 256 and the resampled ROI has at least 16 voxels."""
import numpy as np

from mmnn_sts_amd.data.synth_nifti import ellipsoid_mask

NORM_TPB, NORM_MAX_PARTS, NORM_BATCH, NORM_WRITE_GROUPS = 256, 256, 4, 2048      # NM_TPB, NM_MAX_PARTS, NM_BATCH, NM_WRITE_GROUPS
X_LINES, X_CHUNK, LINE_TPB, LINE_BATCH, Z_RUN = 16, 64, 256, 8, 16               # RS_XL, RS_XC, RS_TPB, RS_BATCH, RS_ZRUN
HORIZON = 40


def _i16(rng, shape):
    return rng.integers(-200, 1800, shape).astype(np.int16)


def _n(scan, scale=(1.0, 0.0), lead=0):
    return dict(scan=scan, scale=scale, lead=lead)


def build_normalize():
    rng = np.random.default_rng(961)
    s = (12, 11, 8)
    return {"int16": _n(_i16(rng, (13, 10, 9))),
            "uint8": _n(rng.integers(0, 256, s).astype(np.uint8)),
            "int16_scaled": _n(_i16(rng, s), scale=(-0.5, 100.0)),
            "float32": _n((rng.standard_normal(s) * 300.0).astype(np.float32)),
            "float64": _n(rng.standard_normal(s) * 300.0),
            "off_boundary": _n(_i16(rng, (13, 10, 9)), lead=2),
            "two_trips": _n(_i16(rng, (67, 33, 31))),
            "batched_strides": _n(_i16(rng, (128, 128, 130)))}


def _r(rng, scan, spacing, to, out, scale=(1.0, 0.0), lead=0):
    return dict(scan=scan, mask=(rng.random(scan.shape) < 0.5).astype(np.uint8), spacing=tuple(float(s) for s in spacing),
                to=tuple(float(s) for s in to), out=tuple(out), scale=scale, lead=lead)


def build_resample():
    rng = np.random.default_rng(962)
    c = {}
    c["anisotropic_to_1mm"] = _r(rng, _i16(rng, (13, 10, 9)), (0.8, 1.1, 5.0), (1, 1, 1), (11, 11, 45))
    c["to_2mm"] = _r(rng, _i16(rng, (12, 11, 8)), (0.9, 0.9, 2.5), (2, 2, 2), (6, 5, 10))
    c["upsample_thin"] = _r(rng, _i16(rng, (5, 7, 2)), (1, 1, 1), (0.5, 0.5, 0.5), (10, 14, 4))
    c["extent_1"] = _r(rng, _i16(rng, (40, 3, 1)), (1, 1, 3), (1.5, 1.5, 1.5), (27, 2, 2))
    c["longer_than_horizon"] = _r(rng, _i16(rng, (70, 3, 2)), (1, 1, 1), (0.75, 0.75, 0.75), (94, 4, 3))
    c["axis_kept"] = _r(rng, _i16(rng, (13, 10, 9)), (0.8, 1.1, 5.0), (1, 1, 0), (11, 11, 9))
    s = (12, 11, 8)
    c["type_uint8"] = _r(rng, rng.integers(0, 256, s).astype(np.uint8), (0.9, 0.9, 2.5), (2, 2, 2), (6, 5, 10))
    c["type_int16_scaled"] = _r(rng, _i16(rng, s), (0.9, 0.9, 2.5), (2, 2, 2), (6, 5, 10), scale=(-0.5, 100.0))
    c["type_float32"] = _r(rng, (rng.standard_normal(s) * 300.0).astype(np.float32), (0.9, 0.9, 2.5), (2, 2, 2), (6, 5, 10))
    c["type_float64"] = _r(rng, rng.standard_normal(s) * 300.0, (0.9, 0.9, 2.5), (2, 2, 2), (6, 5, 10))
    c["off_boundary"] = _r(rng, _i16(rng, (13, 10, 9)), (0.8, 1.1, 5.0), (1, 1, 1), (11, 11, 45), lead=2)
    c["chunk_65"] = _r(rng, _i16(rng, (65, 3, 2)), (1, 1, 1), (0.75, 0.75, 0.75), (87, 4, 3))
    c["chunk_128"] = _r(rng, _i16(rng, (128, 2, 2)), (1, 1, 1), (1.5, 1.5, 1.5), (86, 2, 2))
    c["tiles"] = _r(rng, _i16(rng, (66, 13, 6)), (1, 1, 1), (0.75, 0.75, 0.75), (88, 18, 8))
    return c


def _g(rng, shape, spacing, to, classes=(), glszm=False, mesh=False, sigmas=(), log_bin_width=None):
    return dict(scan=_i16(rng, shape), mask=ellipsoid_mask(shape, rng), spacing=tuple(float(s) for s in spacing), to=tuple(float(s) for s in to),
                classes=tuple(classes), glszm=glszm, mesh=mesh, sigmas=tuple(sigmas), log_bin_width=log_bin_width)


def build_features():
    rng = np.random.default_rng(963)
    return {"anisotropic_to_1mm": _g(rng, (13, 10, 9), (0.8, 1.1, 5.0), (1, 1, 1)),
            "to_2mm": _g(rng, (12, 11, 8), (0.9, 0.9, 2.5), (2, 2, 2)),
            "every_class_to_half_mm": _g(rng, (13, 10, 9), (1, 1, 1), (0.5, 0.5, 0.5), ("glrlm", "gldm", "ngtdm"), True, True, (1.0,), 10.0)}


def affine_of(spacing, origin=(0.0, 0.0, 0.0)):
    a = np.diag([float(s) for s in spacing] + [1.0])
    a[:3, 3] = origin
    return a


NORMALIZE_CASES = build_normalize()
RESAMPLE_CASES = build_resample()
FEATURE_CASES = build_features()
SCALE, BIN_WIDTH = 100.0, 25.0
