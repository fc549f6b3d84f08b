"""Radiomic features of a (scan, mask) pair, extracted on the device: binding of `mmnn_radiomics` (csrc/radiomics.hip), of
`mmnn_radiomics_texture` (csrc/radiomics_texture.hip), of `mmnn_radiomics_zones` (csrc/radiomics_zones.hip), of `mmnn_radiomics_mesh`
(csrc/radiomics_mesh.hip), of `mmnn_log_filter` (csrc/radiomics_filter.hip) and of `mmnn_normalize_scan` and `mmnn_resample_pair`
(csrc/radiomics_resample.hip).

    extract(scan, mask, device)            enqueue one extraction; the result holds device tensors, nothing is read back
    finish(result, affine)                 one read-back -> {feature name: float}: adds TotalEnergy and the voxel-based shape features
    extract_tree(dataset, device, out)     every patient and modality of an image dataset -> a csv (`MRN`, then the features)
    feature_names(classes, glszm, mesh, log_sigma, shell_mm)  the columns: FEATURE_NAMES, then those of the requested texture classes, then
                                           the size-zone ones, then the mesh-based shape ones, then those of the filtered images, then
                                           those of the shells
    log_taps(sigma_mm, spacing)            the radii, taps and weights of one Laplacian-of-Gaussian scale (numpy fp64, host only)
    log_filter(scan, sigma_mm, device)     enqueue the filter; the float32 volume stays on the device
    normalize_scan(scan, device, scale, outliers)   enqueue the whole-scan z-score; the float32 volume stays on the device
    resample_grid(shape, affine, spacing)  the output grid of a resampling (numpy fp64, host only); resample_tables(...) its per-axis tables
    resample_pair(scan, mask, device, spacing)      enqueue the resampling -> (float32 scan with the new affine, uint8 mask)
    python -m mmnn_sts_amd.radiomics --image_loc DIR --key_loc key.csv [--config c.yaml] [--classes glrlm,gldm,ngtdm | all] [--glszm]
                                     [--mesh_shape] [--log_sigma 1,3 [--log_bin_width B]] [--normalize [--normalize_scale S]
                                     [--normalize_outliers K]] [--resample_spacing 1,1,1] [--shell_mm 5,10] --out radiomics.csv

Upstream reads such a csv (`Data: rad_loc`, data/RadiomicsDatasets.py) and leaves its extraction to PyRadiomics; here the table is built
from the very pair the image path ingests, through the same mask routes (NIfTI mask, resampled mask, DICOM mask series, RTSTRUCT, SEG:
`data.ingest.prepare_pair`).  The 47 columns carry PyRadiomics' names and definitions -- 18 first-order, 6 voxel-based shape, 23 GLCM --
in voxel index space (distance 1, no resampling, fixed `bin_width`).  The mesh-based shape features (surface area, sphericity, the
diameters) are behind the switch `mesh_shape` below; the GLCM's MCC is out of scope.  What the numbers are pinned to is the numpy
restatement in tests/_radiomics_ref.py.

`classes` (`Radiomics: classes`, `--classes`; empty by default) adds the columns of further texture classes, computed by a second call on
the same stream from the bin volume the first one left on the device: `glrlm` (16 run-length features), `gldm` (14 dependence features,
alpha 0) and `ngtdm` (5), 82 columns per modality with all three.  These too are pinned to a numpy restatement
(tests/_radiomics_texture_ref.py); **parity with PyRadiomics is unpinned**.

`glszm` (`Radiomics: glszm`, `--glszm`; off by default) is a switch of its own beside `classes`: a third call on the same stream labels
the 26-connected zones of equal bin on the device and appends the 16 size-zone features (`original_glszm_*`) behind the other classes: 63
columns per modality alone, 98 with all three classes.  They are pinned to the numpy / scipy restatement in
tests/_radiomics_zones_ref.py; **parity with PyRadiomics is unpinned** here too.

`mesh` (`Radiomics: mesh_shape`, `--mesh_shape`; off by default) is a fourth call on the same stream: it walks the cells of the ROI's
surface mesh on the device (a triangle table generated from a stated rule, tools/gen_mesh_table.py) and returns the exact integer volume,
the surface area under the scan's 3 x 3 linear part and four squared diameters from a pass over all vertex pairs; `finish` derives the
eight columns `original_shape_MeshVolume` ... `original_shape_Maximum2DDiameterRow`, which follow all the others: 55 columns per
modality with the switch alone, 106 with all classes and `glszm`.  Slice, Column and Row hold the z, y and x index of the scan's array
fixed.  They are pinned to the numpy restatement in tests/_radiomics_mesh_ref.py; **parity with PyRadiomics is unpinned**: its table may
triangulate some configurations differently, and it scales by the spacing alone where this uses the full linear part.  The GLCM's MCC
stays out of scope.

`log_sigma` (`Radiomics: log: {sigma: [1.0, 3.0], bin_width: 25}`, `--log_sigma 1,3`; empty by default) adds a second image type: for
every sigma (in mm, ascending) the scan is filtered on the device by a Laplacian of Gaussian at that physical scale (`log_filter`: the
taps follow the scan's voxel spacing, the column norms of its affine's linear part) and the same extraction calls -- first order and GLCM,
the requested texture classes and `glszm`, never the shape classes -- run on the filtered volume under the same device mask, binned at
`log_bin_width` (the original image's `bin_width` when not given).  Their columns `log-sigma-<sigma>-mm-3D_*` (sigma 3 is written `3-0`)
follow every `original_*` one: 41 per sigma by default, 92 with all classes and `glszm`.  The filter is pinned to the numpy restatement
in tests/_radiomics_log_ref.py, bit for bit, and that one to scipy's `gaussian_filter`; **parity with PyRadiomics is unpinned**: its LoG
is ITK's recursive (IIR) Gaussian, this one a sampled FIR truncated at 4 sigma.

`normalize` and `resample` (`Radiomics: normalize: true | {scale: 100, outliers: 3}`, `--normalize`; `Radiomics: resample: {spacing:
[1, 1, 1]}`, `--resample_spacing 1,1,1`; both off by default) are two pre-steps in PyRadiomics' order.  They are settings, not image
types: no column is added or renamed, only the values change, and with both off nothing changes at all.  `normalize` replaces the scan
by (v - mean) / sd * scale with the mean and sd of the WHOLE scan (`normalize_scan`; `outliers: k` clamps to +-k scale).  The default
scale is 100, not PyRadiomics' 1: with the default `bin_width` of 25 a scale of 1 would put every voxel into one bin.  `resample` brings
scan and mask onto a grid of the stated spacing in mm (`resample_pair`: cubic B-spline for the scan, nearest neighbour for the mask;
an entry of 0 keeps that axis; the corner of the first voxel is kept), so that "distance 1" of the texture classes, the LoG taps, the
shape moments and the mesh all see the new grid and its affine.  Without them every texture feature is computed in voxel index space on
the scanner's own grid and in its own intensity units.  Both are pinned to the numpy restatement in tests/_radiomics_resample_ref.py,
bit for bit, and that one to scipy's `spline_filter` / `map_coordinates`; **parity with PyRadiomics is unpinned**: it is not installed
here, its B-spline is ITK's, and it crops the resampled grid to the ROI's bounding box plus padding where this resamples the whole scan.

`shell_mm` (`Radiomics: shell_mm: [5, 10]`, `--shell_mm 5,10`; empty by default) describes the tissue the tumour sits in: for every width r
(in mm, ascending) `data.ingest.mask_margin` builds on the device the shell of the voxels whose exact Euclidean distance to the mask,
under the voxel spacing of the grid the extraction sees (behind `normalize` / `resample`), is above 0 and at most r, and the same
extraction calls -- first order and GLCM, the requested texture classes and `glszm`, never the shape classes or the mesh -- run on the
unfiltered scan under that shell, binned at `bin_width`.  Their columns `shell-<r>-mm_*` (5 is written `5-0`) follow every `original_*`
and `log-*` one.  Shells of the LoG volumes are out of scope.  A shell that selects no voxel (the mask fills the scan) raises as an empty
ROI does.  The mask step is pinned to the numpy restatement in tests/_mask_margin_ref.py, bit for bit, and that one to scipy's
`distance_transform_edt`.  The distance takes the index axes as orthogonal; a sheared affine is not detected.

STAGES states each call once -- its C symbol, buffers, switch, unpacking and columns -- and `extract`, `finish`, `feature_names` and
`features_of` all read it; `enqueue(result, stage, desc, stream)` makes one call into the buffers a result already has.  One read-back
brings every result block to the host, stacked per image (the original, then each filtered one, sigma ascending, then each shell, width ascending): the first call's block,
then, of the calls that ran, the texture block, the size-zone block and the mesh block.
"""
import argparse
import csv
import ctypes
import logging
import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .exceptions.exceptions import ConfigurationError

logger = logging.getLogger(__name__)

DEFAULT_BIN_WIDTH, DEFAULT_MAX_BINS = 25.0, 256
ORDER_RANKS = ("p10_lo", "p10_hi", "p25_lo", "p25_hi", "p50_lo", "p50_hi", "p75_lo", "p75_hi", "p90_lo", "p90_hi")
DEVICE_FIRSTORDER = ("Energy", "Minimum", "Maximum", "Range", "Mean", "Variance", "Skewness", "Kurtosis", "MeanAbsoluteDeviation",
                     "RootMeanSquared", "10Percentile", "90Percentile", "Median", "InterquartileRange", "RobustMeanAbsoluteDeviation",
                     "Entropy", "Uniformity")
FIRSTORDER = DEVICE_FIRSTORDER + ("TotalEnergy",)
SHAPE = ("VoxelVolume", "MajorAxisLength", "MinorAxisLength", "LeastAxisLength", "Elongation", "Flatness")
GLCM = ("Autocorrelation", "JointAverage", "ClusterProminence", "ClusterShade", "ClusterTendency", "Contrast", "Correlation",
        "DifferenceAverage", "DifferenceEntropy", "DifferenceVariance", "JointEnergy", "JointEntropy", "Imc1", "Imc2", "Idm", "Idmn", "Id",
        "Idn", "InverseVariance", "MaximumProbability", "SumAverage", "SumEntropy", "SumSquares")
GLRLM = ("ShortRunEmphasis", "LongRunEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized", "RunLengthNonUniformity",
         "RunLengthNonUniformityNormalized", "RunPercentage", "GrayLevelVariance", "RunVariance", "RunEntropy", "LowGrayLevelRunEmphasis",
         "HighGrayLevelRunEmphasis", "ShortRunLowGrayLevelEmphasis", "ShortRunHighGrayLevelEmphasis", "LongRunLowGrayLevelEmphasis",
         "LongRunHighGrayLevelEmphasis")
GLDM = ("SmallDependenceEmphasis", "LargeDependenceEmphasis", "GrayLevelNonUniformity", "DependenceNonUniformity",
        "DependenceNonUniformityNormalized", "GrayLevelVariance", "DependenceVariance", "DependenceEntropy", "LowGrayLevelEmphasis",
        "HighGrayLevelEmphasis", "SmallDependenceLowGrayLevelEmphasis", "SmallDependenceHighGrayLevelEmphasis",
        "LargeDependenceLowGrayLevelEmphasis", "LargeDependenceHighGrayLevelEmphasis")
NGTDM = ("Coarseness", "Contrast", "Busyness", "Complexity", "Strength")
GLSZM = ("SmallAreaEmphasis", "LargeAreaEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized", "SizeZoneNonUniformity",
         "SizeZoneNonUniformityNormalized", "ZonePercentage", "GrayLevelVariance", "ZoneVariance", "ZoneEntropy", "LowGrayLevelZoneEmphasis",
         "HighGrayLevelZoneEmphasis", "SmallAreaLowGrayLevelEmphasis", "SmallAreaHighGrayLevelEmphasis", "LargeAreaLowGrayLevelEmphasis",
         "LargeAreaHighGrayLevelEmphasis")
MESH_SHAPE = ("MeshVolume", "SurfaceArea", "SurfaceVolumeRatio", "Sphericity", "Maximum3DDiameter", "Maximum2DDiameterSlice",
              "Maximum2DDiameterColumn", "Maximum2DDiameterRow")
TEXTURE_CLASSES = ("glrlm", "gldm", "ngtdm")
_TEXTURE = {"glrlm": GLRLM, "gldm": GLDM, "ngtdm": NGTDM}
LOG_TRUNCATE = 4.0
DEFAULT_NORMALIZE_SCALE = 100.0
RESAMPLE_ENTRY = np.dtype([("w", "<f8", (4,)), ("i", "<i4", (4,)), ("nearest", "<i4"), ("inside", "<i4")])   # mmnn_resample_entry
_logged_identity = False
_logged_unit_spacing = False


def texture_classes(classes) -> tuple:
    """`classes` (names, a comma-separated string, or 'all') -> the requested texture classes in the fixed order of TEXTURE_CLASSES."""
    if classes is None:
        return ()
    if isinstance(classes, str):
        classes = [c for c in classes.replace(",", " ").split() if c]
    names = [str(c).strip().lower() for c in classes]
    if names == ["all"]:
        return TEXTURE_CLASSES
    unknown = [c for c in names if c not in TEXTURE_CLASSES]
    if unknown:
        raise ConfigurationError(f"radiomics: unknown texture class {', '.join(repr(c) for c in unknown)}: the valid ones are "
                                 + ", ".join(TEXTURE_CLASSES) + (" (the size-zone features have a switch of their own: `Radiomics: glszm: true`, "
                                                                 "`--glszm`)" if "glszm" in unknown else ""))
    return tuple(c for c in TEXTURE_CLASSES if c in names)


def log_sigmas(sigma) -> tuple:
    """`sigma` (numbers, a comma-separated string, one number or None) -> the scales in mm, de-duplicated and ascending."""
    if sigma is None:
        return ()
    if isinstance(sigma, str):
        sigma = [v for v in sigma.replace(",", " ").split() if v]
    elif isinstance(sigma, (int, float)) and not isinstance(sigma, bool):
        sigma = [sigma]
    if not isinstance(sigma, (list, tuple)):
        raise ConfigurationError(f"radiomics: log sigma must be a list of positive finite numbers (mm), got {sigma!r}")
    out = set()
    for v in sigma:
        try:
            f = math.nan if isinstance(v, bool) else float(v)
        except (TypeError, ValueError):
            f = math.nan
        if not (f > 0.0 and f < math.inf):
            raise ConfigurationError(f"radiomics: log sigma {v!r} is not a positive finite number (mm)")
        out.add(f)
    return tuple(sorted(out))


def shell_widths(shell_mm) -> tuple:
    """`shell_mm` (numbers, a comma-separated string, one number or None) -> the shell widths in mm, de-duplicated and ascending."""
    if shell_mm is None:
        return ()
    if isinstance(shell_mm, str):
        shell_mm = [v for v in shell_mm.replace(",", " ").split() if v]
    elif isinstance(shell_mm, (int, float)) and not isinstance(shell_mm, bool):
        shell_mm = [shell_mm]
    if not isinstance(shell_mm, (list, tuple)):
        raise ConfigurationError(f"radiomics: shell_mm must be a list of positive finite numbers (mm), got {shell_mm!r}")
    out = set()
    for v in shell_mm:
        try:
            f = math.nan if isinstance(v, bool) else float(v)
        except (TypeError, ValueError):
            f = math.nan
        if not (f > 0.0 and f < math.inf):
            raise ConfigurationError(f"radiomics: shell width {v!r} is not a positive finite number (mm)")
        out.add(f)
    return tuple(sorted(out))


def shell_image_type(radius_mm) -> str:
    """The column prefix of the shell of `radius_mm` mm, written as `log_image_type` writes a sigma: 5 -> `shell-5-0-mm`."""
    return "shell-" + str(float(radius_mm)).replace(".", "-") + "-mm"


def log_image_type(sigma) -> str:
    """PyRadiomics' name of the LoG image type at `sigma` mm: 3 -> `log-sigma-3-0-mm-3D`, 1.5 -> `log-sigma-1-5-mm-3D`."""
    return "log-sigma-" + str(float(sigma)).replace(".", "-") + "-mm-3D"


def feature_names(classes=(), glszm=False, mesh=False, log_sigma=(), shell_mm=()) -> tuple:
    """FEATURE_NAMES, then `original_glrlm_*`, `original_gldm_*`, `original_ngtdm_*` of the requested classes, then with `glszm`
    `original_glszm_*`, then with `mesh` the eight mesh-based `original_shape_*`; then for every sigma of `log_sigma`, ascending,
    `log-sigma-<sigma>-mm-3D_firstorder_*`, `_glcm_*`, the requested classes and with `glszm` `_glszm_*` (never the shape classes);
    then for every width of `shell_mm`, ascending, the same columns under `shell-<r>-mm_*`."""
    classes, names = texture_classes(classes), ()
    for im in ("original",) + tuple(log_image_type(s) for s in log_sigmas(log_sigma)) + tuple(shell_image_type(r) for r in shell_widths(shell_mm)):
        on = {"classes": classes, "glszm": glszm, "mesh_shape": mesh and im == "original"}
        names += tuple(n for st in STAGES if st.flag is None or on[st.flag] for n in st.names(im, classes))
    return names


@dataclass
class RadiomicsResult:
    """One extraction, still on the device.  `block`: the bytes of mmnn_radiomics_result; `hist` (max_bins,) and `glcm`
    (13, max_bins, max_bins) int32 views of the uint32 counts; `shape`, `affine`: the scan's grid.  With texture classes: `texture`, the
    bytes of mmnn_radiomics_texture_result; `glrlm` (13, max_bins, L), `gldm` and `ngtdm_n` (max_bins, 27) int32 views of the uint32 counts,
    `ngtdm_s` (max_bins, 27) int64; `classes`, the requested ones (the device computes all three).  With `glszm`: `zones`, the bytes of
    mmnn_radiomics_zones_result; `labels` and `sizes` (x * y * z,) and `levels` (max_bins,) int32 views of the uint32 tables.  With `mesh`:
    `mesh`, the bytes of mmnn_radiomics_mesh_result; `mesh_cfg` (256,) int64, the cells per configuration; `linear`, the 3 x 3 linear part
    that was enqueued with the call (the scan's, the identity without an affine).  With `log_sigma`: `log`, a tuple of (sigma, the
    RadiomicsResult of the image filtered at sigma); such a result has `image` set to its image type, `bin_width` the filtered images'
    and `filtered`, the DeviceVolume `log_filter` returned (float32, on the scan's grid), beside `filter_taps`, the taps on the device;
    `filter_workspace`, which the scales of one extraction share, is on the original image's result.  With the pre-steps: `normalize`,
    the (scale, outliers) in force, `normalized`, the DeviceVolume `normalize_scan` returned, and `normalize_block`, the bytes of
    mmnn_normalize_result; `resample`, the requested spacing, `resampled`, the (scan, mask) DeviceVolumes `resample_pair` returned (None
    when every ratio is 1 and the step was skipped), and `resample_tables`, the tables on the device; `pre_workspace`, which the two
    steps share; `source_shape`, the extents before the pre-steps.  `shape` and `affine` are then the resampled grid's.
    With `shell_mm`: `shell`, a tuple of (width in mm, the RadiomicsResult of the unfiltered scan under the shell of that width around
    the mask); such a result has `image` set to its column prefix and `shell_mask`, the DeviceVolume `mask_margin` returned (uint8 0 / 1
    on the grid the extraction sees); `shell_workspace`, which the shells of one extraction share, is on the original image's result."""
    block: torch.Tensor
    hist: torch.Tensor
    glcm: torch.Tensor
    workspace: torch.Tensor
    shape: tuple
    affine: Optional[np.ndarray]
    bin_width: float
    max_bins: int
    texture: Optional[torch.Tensor] = None
    glrlm: Optional[torch.Tensor] = None
    gldm: Optional[torch.Tensor] = None
    ngtdm_n: Optional[torch.Tensor] = None
    ngtdm_s: Optional[torch.Tensor] = None
    texture_workspace: Optional[torch.Tensor] = None
    classes: tuple = ()
    zones: Optional[torch.Tensor] = None
    labels: Optional[torch.Tensor] = None
    sizes: Optional[torch.Tensor] = None
    levels: Optional[torch.Tensor] = None
    zones_workspace: Optional[torch.Tensor] = None
    glszm: bool = False
    mesh: Optional[torch.Tensor] = None
    mesh_cfg: Optional[torch.Tensor] = None
    mesh_workspace: Optional[torch.Tensor] = None
    linear: Optional[np.ndarray] = None
    mesh_shape: bool = False
    image: str = "original"
    log: tuple = ()
    filtered: Optional[object] = None
    filter_taps: Optional[torch.Tensor] = None
    filter_workspace: Optional[torch.Tensor] = None
    normalize: Optional[tuple] = None
    normalized: Optional[object] = None
    normalize_block: Optional[torch.Tensor] = None
    resample: Optional[tuple] = None
    resampled: Optional[tuple] = None
    resample_tables: Optional[torch.Tensor] = None
    pre_workspace: Optional[torch.Tensor] = None
    source_shape: Optional[tuple] = None
    shell: tuple = ()
    shell_mask: Optional[object] = None
    shell_workspace: Optional[torch.Tensor] = None


def workspace_bytes(x: int, y: int, z: int, max_bins: int = DEFAULT_MAX_BINS) -> int:
    return _lib.count("mmnn_radiomics_workspace_bytes", int(x), int(y), int(z), int(max_bins))


def spacing_of(affine) -> Tuple[float, float, float]:
    """The voxel spacing in mm along x, y, z: the column norms of the affine's linear part; (1, 1, 1) without an affine."""
    global _logged_unit_spacing
    if affine is None:
        if not _logged_unit_spacing:
            logger.info("radiomics: a scan without an affine: the LoG scales are in voxels (spacing 1, 1, 1)")
            _logged_unit_spacing = True
        return (1.0, 1.0, 1.0)
    return tuple(float(v) for v in np.sqrt((_linear_of(affine) ** 2).sum(axis=0)))


def log_taps(sigma_mm: float, spacing=(1.0, 1.0, 1.0)):
    """The sampled Laplacian-of-Gaussian kernel of scale `sigma_mm` on a grid of voxel `spacing` (x, y, z, in mm), separated per axis:
    -> (radius[3], taps, weight[3]), numpy fp64.  Per axis a, with s_a its spacing:
        sigma_a = sigma / s_a                       the scale in voxels
        r_a = int(4 sigma_a + 0.5)                  the truncation at 4 sigma, rounded to the nearest sample
        k = -r_a .. r_a;  g = exp(-k^2 / (2 sigma_a^2));  g /= g.sum()                 the smoothing taps, which sum to 1
        d = (k^2 / sigma_a^4 - 1 / sigma_a^2) g                                        the sampled second derivative
        h = d - g d.sum()                           so that h sums to 0 and a constant image filters to 0 (the sampled d alone leaves a
                                                    bias of 6 % of the image mean at sigma_a = 0.6)
        w_a = sigma^2 / s_a^2                       ITK's normalise-across-scale (sigma^2) together with the mm Laplacian (1 / s_a^2)
    `taps` is g_x, h_x, g_y, h_y, g_z, h_z behind each other, as `mmnn_log_filter` reads them: the filtered image is
    sum_a w_a (h_a along a, g along the two other axes).  An axis whose r_a would be 0 or above the library's largest radius raises
    ConfigurationError."""
    sigma = float(sigma_mm)
    if not (sigma > 0.0 and sigma < math.inf):
        raise ConfigurationError(f"radiomics: log sigma {sigma_mm!r} is not a positive finite number (mm)")
    radius, taps, weight = [], [], []
    for axis, s in zip("xyz", spacing):
        s = float(s)
        if not (s > 0.0 and s < math.inf):
            raise ConfigurationError(f"radiomics: log sigma {sigma} mm: the {axis} axis has spacing {s} mm, which is not positive and finite")
        sv = sigma / s
        r = int(LOG_TRUNCATE * sv + 0.5)
        if not 1 <= r <= _lib.LOG_FILTER_MAX_RADIUS:
            raise ConfigurationError(f"radiomics: log sigma {sigma} mm on the {axis} axis (spacing {s} mm) is {sv:.4g} voxels, a kernel radius "
                                     f"of {r}: the filter takes radii 1..{_lib.LOG_FILTER_MAX_RADIUS} (sigma between 0.125 and "
                                     f"{(_lib.LOG_FILTER_MAX_RADIUS + 0.5) / LOG_TRUNCATE:.5g} voxels on every axis)")
        k = np.arange(-r, r + 1, dtype=np.float64)
        g = np.exp(-(k * k) / (2.0 * sv * sv))
        g /= g.sum()
        d = ((k * k) / sv ** 4 - 1.0 / (sv * sv)) * g
        h = d - g * d.sum()
        radius.append(r)
        taps += [g, h]
        weight.append(sigma * sigma / (s * s))
    return np.array(radius, dtype=np.int32), np.concatenate(taps), np.array(weight, dtype=np.float64)


def log_filter(scan, sigma_mm: float, device, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
               taps: Optional[torch.Tensor] = None):
    """Enqueue `mmnn_log_filter` on the current stream of `device`: `scan` (whatever `ingest.upload` takes) filtered by the Laplacian of
    Gaussian of `sigma_mm` under `log_taps`' rule, with the spacing of the scan's affine.  Returns a DeviceVolume of float32 (NIfTI code
    16) with slope 0 (no scaling) and the scan's affine, which `extract` and the ingest take like any scan.  `out`: a contiguous float32
    tensor of x * y * z elements on the device to write; `workspace`: at least `mmnn_log_filter_workspace_bytes` bytes of uint8; `taps`: a
    float64 device tensor of the taps' length to upload them into.  Each is allocated when None."""
    from .data import ingest
    return _enqueue_log_filter(ingest.upload(scan, torch.device(device)), sigma_mm, out, workspace, taps)[0]


def _enqueue_log_filter(scan, sigma_mm, out, workspace, taps):
    """`log_filter` on an uploaded scan -> (the filtered DeviceVolume, the workspace, the taps on the device)."""
    from .data import ingest
    dev = scan.data.device
    x, y, z = scan.shape
    radius, host_taps, weight = log_taps(sigma_mm, spacing_of(scan.affine))
    out = _lib.device_buffer(out, x * y * z, torch.float32, dev, "log_filter")
    workspace = _lib.workspace(workspace, _lib.count("mmnn_log_filter_workspace_bytes", x, y, z), dev, "log_filter")
    taps = _lib.device_buffer(taps, host_taps.size, torch.float64, dev, "log_filter (taps)")
    taps.copy_(torch.from_numpy(host_taps))
    desc = _lib.LogFilterDesc(x, y, z, scan.datatype, float(scan.slope), float(scan.inter), (ctypes.c_int32 * 3)(*radius.tolist()),
                              (ctypes.c_double * 3)(*weight.tolist()))
    _lib.enqueue("mmnn_log_filter", ctypes.byref(desc), scan.data.data_ptr(), taps.data_ptr(), out.data_ptr(), workspace.data_ptr(), device=dev)
    return ingest.DeviceVolume(out.view(torch.uint8), (x, y, z), 16, 0.0, 0.0, scan.affine), workspace, taps


def normalize_settings(normalize) -> Optional[Tuple[float, float]]:
    """`normalize` (None / False, True, a mapping of `scale` and `outliers`, or the pair) -> None or (scale, outliers): the scale is 100
    and outliers 0 (no clamp) when not given."""
    if normalize is None or normalize is False:
        return None
    if normalize is True:
        normalize = {}
    if isinstance(normalize, (list, tuple)) and len(normalize) == 2:
        normalize = {"scale": normalize[0], "outliers": normalize[1]}
    valid = ("radiomics: normalize must be true / false or a mapping of `scale` (a positive finite number, default 100) and `outliers` "
             "(a finite number >= 0; 0: no clamp)")
    if not isinstance(normalize, dict) or set(normalize) - {"scale", "outliers"}:
        raise ConfigurationError(f"{valid}, got {normalize!r}")
    out = []
    for key, default in (("scale", DEFAULT_NORMALIZE_SCALE), ("outliers", 0.0)):
        v = normalize.get(key)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0.0 or (key == "scale" and v == 0.0):
            raise ConfigurationError(f"{valid}, got {key} {v!r}")
        out.append(float(v))
    return tuple(out)


def resample_spacing(resample) -> Optional[Tuple[float, float, float]]:
    """`resample` (None, one number, three numbers, a comma-separated string, or a mapping of `spacing`) -> None or the requested
    spacing along x, y, z in mm; an entry of 0 keeps that axis."""
    if resample is None or resample is False:
        return None
    valid = "radiomics: resample spacing must be one number or three (mm, finite, >= 0; 0 keeps that axis)"
    if isinstance(resample, dict):
        if set(resample) != {"spacing"}:
            raise ConfigurationError(f"radiomics: resample must be a mapping of `spacing` alone, got {resample!r}")
        resample = resample["spacing"]
    if isinstance(resample, str):
        resample = [v for v in resample.replace(",", " ").split() if v]
    elif isinstance(resample, (int, float)) and not isinstance(resample, bool):
        resample = [resample]
    if not isinstance(resample, (list, tuple, np.ndarray)) or len(resample) not in (1, 3):
        raise ConfigurationError(f"{valid}, got spacing {resample!r}")
    out = []
    for v in resample:
        try:
            f = math.nan if isinstance(v, bool) else float(v)
        except (TypeError, ValueError):
            f = math.nan
        if not (math.isfinite(f) and f >= 0.0):
            raise ConfigurationError(f"{valid}, got spacing {v!r}")
        out.append(f)
    return tuple(out * 3) if len(out) == 1 else tuple(out)


class ResampleGrid(NamedTuple):
    """`resample_grid`'s result: `shape`, the output extents; `ratio`, r_a = requested / present spacing per axis; `affine`, the output
    grid's voxel index -> mm matrix; `skip`: every ratio is 1, nothing is to be done."""
    shape: Tuple[int, int, int]
    ratio: np.ndarray
    affine: np.ndarray
    skip: bool


def resample_grid(shape, affine, spacing) -> ResampleGrid:
    """The grid a scan of extents `shape` and voxel index -> mm matrix `affine` (None: the identity) is resampled onto at the requested
    `spacing` (one number or three, mm; 0 keeps that axis).  numpy fp64, host only.  Per axis a, with n_a the extent, s_a the present
    spacing (`spacing_of`), q_a the requested one and r_a = q_a / s_a:
        m_a = max(1, ceil(n_a s_a / q_a - 2^-20))        the output extent
        c_a(j) = (j + 0.5) r_a - 0.5                     the old continuous index of new voxel j: the corner of the first voxel is kept
        A' = A with column a scaled by r_a, translation t + L (0.5 r - 0.5)
    A new voxel is outside (scan 0.0, mask 0) when c_a < -0.5 or c_a >= n_a - 0.5 on any axis, which happens on the last plane of an
    axis when m_a r_a - n_a > 0.5 r_a.  This is the whole scan's grid, not the ROI's bounding box."""
    q = resample_spacing(spacing)
    if q is None:
        raise ConfigurationError(f"radiomics: resample spacing must be given, got {spacing!r}")
    n = np.array([int(v) for v in shape], dtype=np.float64)
    s = np.array(spacing_of(affine), dtype=np.float64)
    if not (np.isfinite(s).all() and (s > 0.0).all()):
        raise ConfigurationError(f"radiomics: resample spacing {q}: the scan's own spacing {tuple(s)} is not positive and finite")
    q = np.where(np.array(q) == 0.0, s, np.array(q, dtype=np.float64))
    r = q / s
    m = np.maximum(1.0, np.ceil(n * s / q - 2.0 ** -20))
    # the output grid and the two intermediates of `mmnn_resample_pair` ([z][y][mx] and [z][my][mx]) must each stay below 2^31 elements
    if max(float(np.prod(m)), float(m[0] * n[1] * n[2]), float(m[0] * m[1] * n[2])) >= 2.0 ** 31:
        raise ConfigurationError(f"radiomics: resample spacing {tuple(q)} mm turns the scan of {tuple(int(v) for v in n)} voxels at "
                                 f"{tuple(s)} mm into {tuple(int(v) for v in m)}: 2^31 voxels or more in the output or in an intermediate "
                                 "of the separable passes")
    A = np.eye(4) if affine is None else np.array(affine, dtype=np.float64)
    if A.shape == (3, 3):
        A = np.block([[A, np.zeros((3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]])
    out = A.copy()
    out[:3, :3] = A[:3, :3] * r[None, :]
    out[:3, 3] = A[:3, 3] + A[:3, :3] @ (0.5 * r - 0.5)
    return ResampleGrid(tuple(int(v) for v in m), r, out, bool((r == 1.0).all()))


def resample_tables(shape, grid: ResampleGrid) -> np.ndarray:
    """The per-axis tables of `mmnn_resample_pair` for a scan of extents `shape` and the grid of `resample_grid`: a structured array
    (RESAMPLE_ENTRY, 56 bytes per entry) of the x axis' entries, then y's, then z's.  Entry j of an axis of extent n: c = (j + 0.5) r -
    0.5, f = floor(c), t = c - f; `i`: mirror(f - 1 + k), k = 0..3, whole-sample symmetric with period 2 n - 2 (0 for n = 1); `w`: the
    cubic B-spline weights (1-t)^3/6, 2/3 - t^2 (2-t)/2, 2/3 - (1-t)^2 (1+t)/2, t^3/6; `nearest`: clamp(floor(c + 0.5), 0, n - 1);
    `inside`: not (c < -0.5 or c >= n - 0.5)."""
    parts = []
    for n, m, r in zip(shape, grid.shape, grid.ratio):
        n = int(n)
        c = (np.arange(m, dtype=np.float64) + 0.5) * float(r) - 0.5
        f = np.floor(c)
        t, u = c - f, 1.0 - (c - f)
        e = np.zeros(m, dtype=RESAMPLE_ENTRY)
        i = f.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :]
        if n == 1:
            i[:] = 0
        else:
            i = np.mod(i, 2 * n - 2)
            i = np.where(i < n, i, 2 * n - 2 - i)
        e["i"] = i
        e["w"] = np.stack([u * u * u / 6.0, 2.0 / 3.0 - t * t * (2.0 - t) / 2.0, 2.0 / 3.0 - u * u * (1.0 + t) / 2.0, t * t * t / 6.0], axis=1)
        e["nearest"] = np.clip(np.floor(c + 0.5), 0, n - 1).astype(np.int64)
        e["inside"] = ~((c < -0.5) | (c >= n - 0.5))
        parts.append(e)
    return np.concatenate(parts)


def resample_constants() -> dict:
    """What the prefilter's recursion takes from the descriptor: the pole z = sqrt(3) - 2, z / (z^2 - 1), the gain 6 and z^k for k below
    the horizon."""
    z = math.sqrt(3.0) - 2.0
    return {"pole": z, "pole_gain": z / (z * z - 1.0), "gain": 6.0, "pole_power": np.array([z ** k for k in range(_lib.RESAMPLE_HORIZON)])}


def normalize_scan(scan, device, scale: float = DEFAULT_NORMALIZE_SCALE, outliers: float = 0.0, out: Optional[torch.Tensor] = None,
                   block: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Enqueue `mmnn_normalize_scan` on the current stream of `device`: `scan` (whatever `ingest.upload` takes) becomes
    (v - mean) / sd * scale with the mean and the sd (divisor n - 1) of the whole scan, clamped to +-outliers * scale when `outliers` > 0.
    Returns (a DeviceVolume of float32 (NIfTI code 16) with slope 0 and the scan's affine, the device's result block -- n, mean, sd,
    nonfinite: `unpack_normalize` -- which stays there).  `out`: x * y * z contiguous float32 on the device; `block`:
    NORMALIZE_RESULT_BYTES of uint8; `workspace`: at least `mmnn_normalize_scan_workspace_bytes` of uint8.  Each is allocated when None."""
    from .data import ingest
    settings = normalize_settings({"scale": scale, "outliers": outliers})
    return _enqueue_normalize(ingest.upload(scan, torch.device(device)), settings, out, block, workspace)[:2]


def unpack_normalize(raw: np.ndarray) -> dict:
    """The bytes of mmnn_normalize_result -> its fields."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    return {"n": int(raw[:8].view(np.int64)[0]), "mean": float(raw[8:16].view(np.float64)[0]), "sd": float(raw[16:24].view(np.float64)[0]),
            "nonfinite": bool(raw[24:32].view(np.int64)[0])}


def _enqueue_normalize(scan, settings, out, block, workspace):
    """`normalize_scan` on an uploaded scan -> (the normalised DeviceVolume, the result block, the workspace)."""
    from .data import ingest
    dev = scan.data.device
    x, y, z = scan.shape
    out = _lib.device_buffer(out, x * y * z, torch.float32, dev, "normalize_scan")
    block = _lib.device_buffer(block, _lib.NORMALIZE_RESULT_BYTES, torch.uint8, dev, "normalize_scan (result block)")
    workspace = _lib.workspace(workspace, _lib.count("mmnn_normalize_scan_workspace_bytes", x, y, z), dev, "normalize_scan")
    desc = _lib.NormalizeDesc(x, y, z, scan.datatype, float(scan.slope), float(scan.inter), settings[0], settings[1])
    _lib.enqueue("mmnn_normalize_scan", ctypes.byref(desc), scan.data.data_ptr(), out.data_ptr(), block.data_ptr(), workspace.data_ptr(), device=dev)
    return ingest.DeviceVolume(out.view(torch.uint8), (x, y, z), 16, 0.0, 0.0, scan.affine), block, workspace


def resample_workspace_bytes(shape, out_shape) -> int:
    return _lib.count("mmnn_resample_pair_workspace_bytes", *(int(v) for v in (*shape, *out_shape)))


def resample_pair(scan, mask, device, spacing, index_map=None, threshold: Optional[float] = None, out: Optional[torch.Tensor] = None,
                  out_mask: Optional[torch.Tensor] = None, tables: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Enqueue `mmnn_resample_pair` on the current stream of `device`: the pair (whatever `ingest.prepare_pair` takes) is brought onto
    the grid `resample_grid` gives for `spacing`, the scan by cubic B-spline interpolation, the mask by nearest neighbour.  Returns two
    DeviceVolumes with the new affine: float32 (NIfTI code 16, slope 0) and uint8 (0 / 1).  When every ratio is 1 the prepared pair is
    returned as it is.  `out` / `out_mask`: contiguous float32 / uint8 tensors of the output's voxel count; `tables`: uint8 of 56 bytes
    per entry to upload the tables into; `workspace`: at least `resample_workspace_bytes` of uint8.  Each is allocated when None."""
    from .data import ingest
    scan, mask = ingest.prepare_pair(scan, mask, torch.device(device), index_map, threshold, what="radiomics")
    grid = resample_grid(scan.shape, scan.affine, spacing)
    if grid.skip:
        return scan, mask
    return _enqueue_resample(scan, mask, grid, out, out_mask, tables, workspace)[:2]


def _enqueue_resample(scan, mask, grid, out, out_mask, tables, workspace):
    """`resample_pair` on a prepared pair -> (the scan's DeviceVolume, the mask's, the tables on the device, the workspace)."""
    from .data import ingest
    dev = scan.data.device
    (x, y, z), (mx, my, mz) = scan.shape, grid.shape
    host = resample_tables(scan.shape, grid)
    out = _lib.device_buffer(out, mx * my * mz, torch.float32, dev, "resample_pair")
    out_mask = _lib.device_buffer(out_mask, mx * my * mz, torch.uint8, dev, "resample_pair (mask)")
    tables = _lib.device_buffer(tables, host.nbytes, torch.uint8, dev, "resample_pair (tables)")
    workspace = _lib.workspace(workspace, resample_workspace_bytes(scan.shape, grid.shape), dev, "resample_pair")
    tables.copy_(torch.from_numpy(host.view(np.uint8)))
    k = resample_constants()
    desc = _lib.ResampleDesc(x, y, z, mx, my, mz, scan.datatype, mask.datatype, float(scan.slope), float(scan.inter), float(mask.slope),
                             float(mask.inter), k["pole"], k["pole_gain"], k["gain"], (ctypes.c_double * _lib.RESAMPLE_HORIZON)(*k["pole_power"].tolist()))
    _lib.enqueue("mmnn_resample_pair", ctypes.byref(desc), scan.data.data_ptr(), mask.data.data_ptr(), host.ctypes.data, tables.data_ptr(),
                 out.data_ptr(), out_mask.data_ptr(), workspace.data_ptr(), device=dev)
    return (ingest.DeviceVolume(out.view(torch.uint8), grid.shape, 16, 0.0, 0.0, grid.affine),
            ingest.DeviceVolume(out_mask, grid.shape, 2, 1.0, 0.0, grid.affine), tables, workspace)


def _pre_steps(scan, mask, norm, spacing, buffers):
    """The pre-steps of one extraction on the prepared pair, in PyRadiomics' order: normalise, then resample.  Returns the pair the calls
    are to see and what the result records of the steps: {RadiomicsResult attribute: value}, empty with both off."""
    old = None if buffers is None else (buffers.normalize, buffers.resample, buffers.source_shape)
    if old is not None and old != (norm, spacing, tuple(scan.shape) if norm or spacing else None):
        raise ValueError(f"radiomics: buffers of the pre-steps normalize {old[0]}, resample {old[1]} on a scan of {old[2]} cannot take an "
                         f"extraction with normalize {norm}, resample {spacing} on a scan of {tuple(scan.shape)}")
    if not (norm or spacing):
        return scan, mask, {}
    rec = {"normalize": norm, "resample": spacing, "source_shape": tuple(scan.shape)}
    grid = None if spacing is None else resample_grid(scan.shape, scan.affine, spacing)
    grid = None if grid is None or grid.skip else grid
    if buffers is not None:
        ws = buffers.pre_workspace
    else:
        need = max(_lib.count("mmnn_normalize_scan_workspace_bytes", *scan.shape) if norm else 0,
                   resample_workspace_bytes(scan.shape, grid.shape) if grid is not None else 0)
        ws = torch.empty(need, dtype=torch.uint8, device=scan.data.device) if need else None
    rec["pre_workspace"] = ws
    if norm:
        prev = None if buffers is None else buffers.normalized.data.view(torch.float32)
        scan, rec["normalize_block"], _ = _enqueue_normalize(scan, norm, prev, None if buffers is None else buffers.normalize_block, ws)
        rec["normalized"] = scan
    if grid is not None:
        if buffers is not None and buffers.resampled is None:
            raise ValueError(f"radiomics: buffers of a skipped resampling (every ratio 1) cannot take one onto {grid.shape}")
        prev = (None, None, None) if buffers is None else (buffers.resampled[0].data.view(torch.float32), buffers.resampled[1].data, buffers.resample_tables)
        scan, mask, rec["resample_tables"], _ = _enqueue_resample(scan, mask, grid, *prev, ws)
        rec["resampled"] = (scan, mask)
    return scan, mask, rec


def extract(scan, mask, device, bin_width: float = DEFAULT_BIN_WIDTH, max_bins: int = DEFAULT_MAX_BINS, index_map=None,
            threshold: Optional[float] = None, buffers: Optional[RadiomicsResult] = None, classes=(), glszm: bool = False,
            mesh: bool = False, log_sigma=(), log_bin_width: Optional[float] = None, normalize=None, resample=None,
            shell_mm=()) -> RadiomicsResult:
    """Enqueue the extraction of one (scan, mask) pair on the current stream of `device`.  `scan` / `mask`: whatever `ingest_volume`
    takes (host volumes are uploaded; a contour, SEG or other-grid mask is brought onto the scan's grid first, `index_map` and
    `threshold` as there).  `buffers`: a former result of the same extents and `max_bins` whose tensors are written again.  `classes`:
    texture classes of TEXTURE_CLASSES; when not empty `mmnn_radiomics_texture` is enqueued behind the extraction.  `glszm`: enqueue
    `mmnn_radiomics_zones` behind them.  `mesh`: enqueue `mmnn_radiomics_mesh` behind those, with the linear part of the scan's affine (the
    identity without one), which the result remembers.  `log_sigma`: LoG scales in mm; behind the original image's calls, for each sigma
    ascending, `log_filter` and then the same calls but the mesh one on the filtered volume, under the same prepared mask and binned at
    `log_bin_width` (None: `bin_width`); the results are `RadiomicsResult.log`.  `buffers` must then come from an extraction with the
    same scales.  `normalize` (`normalize_settings`) and `resample` (`resample_spacing`): the pre-steps, enqueued in this order behind
    `ingest.prepare_pair` and ahead of every call, which then see the new pair and its affine; `buffers` must come from an extraction with
    the same settings on the same extents.  With both None nothing is enqueued or allocated for them.  `shell_mm`: shell widths in mm;
    behind every other call, for each width ascending, `ingest.mask_margin` builds the shell of that width around the mask (mode 'shell':
    within the width of the mask but not of it) on the grid the calls see -- behind the pre-steps, with that grid's spacing -- and the
    same calls but the mesh one run on the unfiltered scan under it, binned at `bin_width`; the results are `RadiomicsResult.shell`.  No
    shell of a filtered volume is taken.  `buffers` must then come from an extraction with the same widths.  Empty: nothing is enqueued
    or allocated for it."""
    from .data import ingest
    dev = torch.device(device)
    scan, mask = ingest.prepare_pair(scan, mask, dev, index_map, threshold, what="radiomics")
    classes, sigmas, shells = texture_classes(classes), log_sigmas(log_sigma), shell_widths(shell_mm)
    if buffers is not None and tuple(r for r, _ in buffers.shell) != shells:
        raise ValueError(f"radiomics: buffers of the shell widths {tuple(r for r, _ in buffers.shell)} cannot take an extraction at {shells}")
    if buffers is not None and tuple(s for s, _ in buffers.log) != sigmas:
        raise ValueError(f"radiomics: buffers of the LoG scales {tuple(s for s, _ in buffers.log)} cannot take an extraction at {sigmas}")
    scan, mask, pre = _pre_steps(scan, mask, normalize_settings(normalize), resample_spacing(resample), buffers)
    out = _extract_image(scan, mask, bin_width, max_bins, buffers, classes, glszm, mesh)
    for k, v in pre.items():
        setattr(out, k, v)
    if sigmas:
        out.filter_workspace = None if buffers is None else buffers.filter_workspace
        subs = []
        for i, s in enumerate(sigmas):
            old = None if buffers is None else buffers.log[i][1]
            vol, out.filter_workspace, taps = _enqueue_log_filter(scan, s, None if old is None else old.filtered.data.view(torch.float32),
                                                                  out.filter_workspace, None if old is None else old.filter_taps)
            sub = _extract_image(vol, mask, bin_width if log_bin_width is None else log_bin_width, max_bins, old, classes, glszm, False)
            sub.image, sub.filtered, sub.filter_taps = log_image_type(s), vol, taps
            subs.append((s, sub))
        out.log = tuple(subs)
    if shells:
        out.shell_workspace = None if buffers is None else buffers.shell_workspace
        if out.shell_workspace is None:
            out.shell_workspace = torch.empty(ingest.mask_margin_workspace_bytes(*scan.shape), dtype=torch.uint8, device=scan.data.device)
        subs = []
        for i, r in enumerate(shells):
            old = None if buffers is None else buffers.shell[i][1]
            rim = ingest.mask_margin(mask, spacing_of(scan.affine), r, "shell", None if old is None else old.shell_mask.data,
                                     workspace=out.shell_workspace)
            rim.affine = scan.affine
            sub = _extract_image(scan, rim, bin_width, max_bins, old, classes, glszm, False)
            sub.image, sub.shell_mask = shell_image_type(r), rim
            subs.append((r, sub))
        out.shell = tuple(subs)
    return out


def _extract_image(scan, mask, bin_width, max_bins, buffers, classes, glszm, mesh) -> RadiomicsResult:
    """The calls of one image (the original scan or a filtered volume) under the prepared device mask."""
    x, y, z = scan.shape
    max_bins = int(max_bins)
    if buffers is not None and (tuple(buffers.shape) != (x, y, z) or buffers.max_bins != max_bins or buffers.block.device != scan.data.device):
        raise ValueError(f"radiomics: buffers of extent {buffers.shape} / {buffers.max_bins} bins cannot take a scan of {(x, y, z)} / {max_bins}")
    desc = _lib.RadiomicsDesc(x, y, z, scan.datatype, mask.datatype, float(scan.slope), float(scan.inter), float(mask.slope), float(mask.inter),
                              float(bin_width), max_bins)
    out = RadiomicsResult(None, None, None, None, (x, y, z), scan.affine, float(bin_width), max_bins)
    for st, on in zip(STAGES, (True, classes, glszm, mesh)):
        if on:
            _enqueue_stage(out, st, desc, buffers, scan.data, mask.data)
            if st.flag is not None:
                setattr(out, st.flag, classes if st.flag == "classes" else True)
    return out


def _enqueue_stage(out: RadiomicsResult, st, desc, buffers, scan, mask) -> None:
    """Give `out` the buffers of stage `st`, those of `buffers` when it has them and new ones otherwise, and enqueue the stage."""
    if buffers is not None and getattr(buffers, st.block) is not None:
        for a in st.attrs:
            setattr(out, a, getattr(buffers, a))
    else:
        (x, y, z), dev = out.shape, scan.device
        nbytes = _lib.count(st.symbol + "_workspace_bytes", x, y, z, out.max_bins)
        setattr(out, st.block, torch.empty(st.nbytes, dtype=torch.uint8, device=dev))
        for a, shape, dtype in st.tables:
            setattr(out, a, torch.empty(shape(x, y, z, out.max_bins), dtype=dtype, device=dev))
        setattr(out, st.workspace, torch.empty(nbytes, dtype=torch.uint8, device=dev))
    if st.name == "mesh":
        out.linear = _linear_of(out.affine)
    _lib.enqueue(st.symbol, *_stage_args(out, st, desc, scan.data_ptr(), mask.data_ptr()), device=scan.device)


def _stage_args(r: RadiomicsResult, st, desc, scan, mask) -> tuple:
    """The arguments of stage `st`'s call ahead of its stream."""
    lead = (scan, mask) if st.flag is None else (r.block.data_ptr(), r.workspace.data_ptr()) + st.extra(r)
    return (ctypes.byref(desc), *lead, *(getattr(r, a).data_ptr() for a in st.attrs))


def enqueue(r: RadiomicsResult, stage: str, desc, stream, scan: Optional[int] = None, mask: Optional[int] = None) -> None:
    """Enqueue the call of one stage of STAGES (`first`, `texture`, `zones`, `mesh`) into the buffers `r` already has, under the
    descriptor `desc` on `stream` (the current device's): nothing is prepared or allocated.  `scan` / `mask`: the device addresses the
    first call reads; the follow-on calls read `r.block` and `r.workspace`, the mesh one `r.linear` too."""
    st = _STAGE[stage]
    _lib.call(st.symbol, *_stage_args(r, st, desc, scan, mask), stream)


def _linear_of(affine) -> np.ndarray:
    """The 3 x 3 linear part of a voxel index -> mm matrix (4 x 4, or 3 x 3 as it is); the identity for None."""
    return np.eye(3) if affine is None else np.ascontiguousarray(np.asarray(affine, dtype=np.float64)[:3, :3])


def mesh_table() -> dict:
    """The triangle table the library was built with (host only, no device): `tri` (256, 16) int8, `l48` (256,), `nsum` (256, 3) int32."""
    tri = np.zeros((_lib.RADIOMICS_MESH_CONFIGS, _lib.RADIOMICS_MESH_TRI_ROW), dtype=np.int8)
    l48, nsum = np.zeros(_lib.RADIOMICS_MESH_CONFIGS, dtype=np.int32), np.zeros((_lib.RADIOMICS_MESH_CONFIGS, 3), dtype=np.int32)
    _lib.call("mmnn_radiomics_mesh_table", tri.ctypes.data, l48.ctypes.data, nsum.ctypes.data)
    return {"tri": tri, "l48": l48, "nsum": nsum}


def unpack_mesh(raw: np.ndarray) -> dict:
    """The bytes of mmnn_radiomics_mesh_result -> its fields."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    i, f = raw[:24].view(np.int64), raw[24:].view(np.float64)
    out = {k: int(v) for k, v in zip(("n_vertices", "n_triangles", "volume48"), i)}
    out["area"], out["q"] = float(f[0]), f[1:5].copy()
    return out


def mesh_features(mesh: dict, linear) -> Dict[str, float]:
    """The eight mesh-based shape features from the device's block: MeshVolume = volume48 / 48 |det L|, SurfaceArea as returned,
    SurfaceVolumeRatio = A / V, Sphericity = (36 pi V^2)^(1/3) / A, each diameter sqrt(q) / 2."""
    V = mesh["volume48"] / 48.0 * abs(float(np.linalg.det(np.asarray(linear, dtype=np.float64).reshape(3, 3))))
    A = mesh["area"]
    out = {"MeshVolume": V, "SurfaceArea": A, "SurfaceVolumeRatio": A / V if V > 0.0 else float("nan"),
           "Sphericity": (36.0 * math.pi * V * V) ** (1.0 / 3.0) / A if A > 0.0 else float("nan")}
    for n, q in zip(MESH_SHAPE[4:], mesh["q"]):
        out[n] = math.sqrt(float(q)) / 2.0
    return out


def unpack_texture(raw: np.ndarray) -> dict:
    """The bytes of mmnn_radiomics_texture_result -> its fields."""
    f = np.ascontiguousarray(raw, dtype=np.uint8).view(np.float64)
    a, b = _lib.RADIOMICS_GLRLM, _lib.RADIOMICS_GLRLM + _lib.RADIOMICS_GLDM
    return {"glrlm": f[:a].copy(), "gldm": f[a:b].copy(), "ngtdm": f[b:].copy()}


def unpack_zones(raw: np.ndarray) -> dict:
    """The bytes of mmnn_radiomics_zones_result -> its fields."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    i, f = raw[:48].view(np.int64), raw[48:].view(np.float64)
    out = {k: int(v) for k, v in zip(("nz", "n_keys", "max_size", "sum_pg2", "sum_ps2", "sum_j2"), i)}
    out["glszm"] = f.copy()
    return out


def unpack_block(raw: np.ndarray) -> dict:
    """The bytes of mmnn_radiomics_result -> its fields."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    ni = _lib.RADIOMICS_RESULT_INT64
    i, f = raw[:ni * 8].view(np.int64), raw[ni * 8:].view(np.float64)
    return {"n": int(i[0]), "lo": i[1:4].copy(), "hi": i[4:7].copy(), "moments": i[7:16].copy(), "n_bins": int(i[16]),
            "overflow": bool(i[17]), "nonfinite": bool(i[18]), "empty": bool(i[19]), "order": f[:10].copy(),
            "firstorder": f[10:10 + _lib.RADIOMICS_FIRSTORDER].copy(), "glcm": f[10 + _lib.RADIOMICS_FIRSTORDER:].copy()}


def shape_features(n: int, moments, linear) -> Dict[str, float]:
    """The six voxel-based shape features from the exact integer sums: VoxelVolume = n |det L|; the axis lengths 4 sqrt(lambda) of the
    eigenvalues of L Cov_idx L^T (population covariance of the ROI's voxel indices), Elongation and Flatness their ratios."""
    L = np.asarray(linear, dtype=np.float64).reshape(3, 3)
    sx, sy, sz, sxx, syy, szz, sxy, sxz, syz = (int(v) for v in moments)
    s1 = (sx, sy, sz)
    s2 = ((sxx, sxy, sxz), (sxy, syy, syz), (sxz, syz, szz))
    # n^2 Cov = n * S2 - S1 S1^T, exact in Python integers
    cov = np.array([[(n * s2[a][b] - s1[a] * s1[b]) for b in range(3)] for a in range(3)], dtype=object)
    cov = np.array([[float(cov[a][b]) for b in range(3)] for a in range(3)], dtype=np.float64) / (float(n) * float(n))
    lam = np.sort(np.linalg.eigvalsh(L @ cov @ L.T))[::-1]
    lam = np.maximum(lam, 0.0)
    out = {"VoxelVolume": n * abs(float(np.linalg.det(L)))}
    for name, v in zip(("MajorAxisLength", "MinorAxisLength", "LeastAxisLength"), lam):
        out[name] = 4.0 * math.sqrt(v)
    out["Elongation"] = math.sqrt(lam[1] / lam[0]) if lam[0] > 0.0 else float("nan")
    out["Flatness"] = math.sqrt(lam[2] / lam[0]) if lam[0] > 0.0 else float("nan")
    return out


@dataclass(frozen=True)
class Stage:
    """One call of an extraction, stated once.  `symbol`: the C function (its workspace size is `<symbol>_workspace_bytes`); `block`: the
    RadiomicsResult attribute of its result block of `nbytes` bytes; `tables`: its caller-owned tables as (attribute, shape from x, y, z,
    max_bins, dtype); `workspace`: the attribute of its workspace; `flag`: the attribute in which a result records that the call ran (None:
    the first call, which always runs); `unpack`: the block's bytes -> its fields; `names(image, classes)`: its columns in order, and
    `values(fields, classes, linear, image)` their values; `extra(result)`: arguments between the first call's workspace and the block."""
    name: str
    symbol: str
    block: str
    nbytes: int
    tables: tuple
    workspace: str
    flag: Optional[str]
    unpack: object
    names: object
    values: object
    extra: object = lambda r: ()

    @property
    def attrs(self) -> tuple:
        """The attributes of the buffers in the order of the C arguments: block, tables, workspace."""
        return (self.block,) + tuple(t[0] for t in self.tables) + (self.workspace,)


def _first_names(image, classes=()):
    return (tuple(f"{image}_firstorder_{n}" for n in FIRSTORDER) + (tuple(f"original_shape_{n}" for n in SHAPE) if image == "original" else ())
            + tuple(f"{image}_glcm_{n}" for n in GLCM))


def _first_values(f, classes, linear, image):
    fo = [float(v) for v in f["firstorder"]]
    shape = shape_features(f["n"], f["moments"], linear) if image == "original" else None
    return (fo + [fo[DEVICE_FIRSTORDER.index("Energy")] * abs(float(np.linalg.det(linear)))] + ([shape[n] for n in SHAPE] if shape else [])
            + [float(v) for v in f["glcm"]])


_NBHD = lambda x, y, z, mb: (mb, _lib.RADIOMICS_NEIGHBOURS)
_VOXELS = lambda x, y, z, mb: (x * y * z,)
STAGES = (
    Stage("first", "mmnn_radiomics", "block", _lib.RADIOMICS_RESULT_BYTES,
          (("hist", lambda x, y, z, mb: (mb,), torch.int32), ("glcm", lambda x, y, z, mb: (_lib.RADIOMICS_DIRECTIONS, mb, mb), torch.int32)),
          "workspace", None, unpack_block, _first_names, _first_values),
    Stage("texture", "mmnn_radiomics_texture", "texture", _lib.RADIOMICS_TEXTURE_BYTES,
          (("glrlm", lambda x, y, z, mb: (_lib.RADIOMICS_DIRECTIONS, mb, max(x, y, z)), torch.int32), ("gldm", _NBHD, torch.int32),
           ("ngtdm_n", _NBHD, torch.int32), ("ngtdm_s", _NBHD, torch.int64)),
          "texture_workspace", "classes", unpack_texture,
          lambda image, classes: tuple(f"{image}_{c}_{n}" for c in classes for n in _TEXTURE[c]),
          lambda f, classes, linear, image: [float(v) for c in classes for v in f[c]]),
    Stage("zones", "mmnn_radiomics_zones", "zones", _lib.RADIOMICS_ZONES_BYTES,
          (("labels", _VOXELS, torch.int32), ("sizes", _VOXELS, torch.int32), ("levels", lambda x, y, z, mb: (mb,), torch.int32)),
          "zones_workspace", "glszm", unpack_zones,
          lambda image, classes: tuple(f"{image}_glszm_{n}" for n in GLSZM),
          lambda f, classes, linear, image: [float(v) for v in f["glszm"]]),
    Stage("mesh", "mmnn_radiomics_mesh", "mesh", _lib.RADIOMICS_MESH_BYTES,
          (("mesh_cfg", lambda x, y, z, mb: (_lib.RADIOMICS_MESH_CONFIGS,), torch.int64),),
          "mesh_workspace", "mesh_shape", unpack_mesh,
          lambda image, classes: tuple(f"original_shape_{n}" for n in MESH_SHAPE),
          lambda f, classes, linear, image: [mesh_features(f, linear)[n] for n in MESH_SHAPE],
          lambda r: ((ctypes.c_double * 9)(*r.linear.ravel().tolist()),)),
)
_STAGE = {st.name: st for st in STAGES}
FEATURE_NAMES = _first_names("original")


def features_of(fields: dict, affine, what: str = "radiomics", texture: Optional[dict] = None, classes=(), zones: Optional[dict] = None,
                mesh: Optional[dict] = None, image: str = "original", normalized: bool = False) -> Dict[str, float]:
    """The host half of `finish`, from the unpacked block (and, with `classes`, the unpacked texture block; with `zones`, the unpacked
    size-zone block; with `mesh`, the unpacked mesh block, whose area and diameters were computed under the linear part of `affine`).
    `image`: the image type that prefixes the columns; a filtered one has no shape columns and is named in what a flag raises.
    `normalized`: the scan went through `normalize`, which the non-finite flag's message then names."""
    global _logged_identity
    if image != "original":
        what = f"{what}, image type {image}"
    if fields["empty"]:
        raise ConfigurationError(f"{what}: the mask selects no voxel of the scan")
    if fields["nonfinite"]:
        raise ConfigurationError(f"{what}: a NaN or infinite voxel value lies inside the mask" + (
            " (with `normalize` on -- Radiomics: normalize, --normalize -- a NaN or infinite voxel anywhere in the scan, or a constant scan "
            "of an integer type, makes every normalised value NaN)" if normalized else ""))
    if fields["overflow"]:
        raise ConfigurationError(f"{what}: the values inside the mask span {fields['n_bins']} bins, more than max_bins: choose a larger "
                                 + ("bin_width (Radiomics: bin_width)" if image == "original" or image.startswith("shell-") else
                                    "log.bin_width (Radiomics: log: bin_width, --log_bin_width)") + " or more bins (Radiomics: max_bins)")
    if affine is None:
        if not _logged_identity:
            logger.info("radiomics: a scan without an affine: shape features in voxel units (the identity)")
            _logged_identity = True
        linear = np.eye(3)
    else:
        linear = np.asarray(affine, dtype=np.float64)[:3, :3]
    classes, out = texture_classes(classes), {}
    for st, f in zip(STAGES, (fields, texture, zones, mesh)):
        if f is not None:
            out.update(zip(st.names(image, classes), st.values(f, classes, linear, image)))
    return out


def _stage_blocks(r: RadiomicsResult):
    """(the RadiomicsResult of an image, stage, that stage's block) in the order of the stacked read-back: per image -- `r`, then its
    filtered ones, sigma ascending, then its shells, width ascending -- the first call's block, then those of the follow-on calls that ran."""
    for q in (r,) + tuple(sub for _, sub in r.log) + tuple(sub for _, sub in r.shell):
        for st in STAGES:
            if st.flag is None or getattr(q, st.flag):
                yield q, st, getattr(q, st.block)


def _stacked(r: RadiomicsResult) -> torch.Tensor:
    """The result blocks of one extraction behind each other: what one read-back brings to the host."""
    parts = [block for _, _, block in _stage_blocks(r)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _features_of_stacked(raw: np.ndarray, r: RadiomicsResult, affine, what: str) -> Dict[str, float]:
    if r.mesh_shape and not np.array_equal(_linear_of(affine), r.linear):
        raise ValueError(f"{what}: the mesh-based shape features were enqueued under the linear part {r.linear.tolist()}; `finish` cannot "
                         f"apply another one ({_linear_of(affine).tolist()}): extract with the affine that is meant")
    unpacked, off = {}, 0
    for q, st, _ in _stage_blocks(r):
        unpacked.setdefault(id(q), (q, {}))[1][st.name] = st.unpack(raw[off:off + st.nbytes])
        off += st.nbytes
    out = {}
    for q, f in unpacked.values():
        out.update(features_of(f.pop("first"), affine, what, classes=q.classes, image=q.image, normalized=r.normalize is not None, **f))
    return out


def finish(result: RadiomicsResult, affine="scan", what: str = "radiomics") -> Dict[str, float]:
    """One read-back of the result block(s) -> {name: float} over FEATURE_NAMES, then the columns of the result's texture classes, with
    `glszm` the size-zone ones and with `mesh` the mesh-based shape ones (ValueError when `affine` is passed and its linear part is not the
    one the mesh call was enqueued with), then the columns of the result's filtered images.  `affine`: the scan's voxel index -> mm
    matrix (4x4 or its 3x3 linear part as the top-left block), None for the identity; the default takes the scan's own.  A flag raises
    ConfigurationError with the cause, and names the image type when a filtered image set it."""
    if isinstance(affine, str):
        affine = result.affine
    return _features_of_stacked(_stacked(result).cpu().numpy(), result, affine, what)


def _volumes_of(dataset, patient):
    return dataset._volumes(patient) if hasattr(dataset, "_volumes") else [dataset._load(patient)]


def extract_tree(dataset, device, out_path=None, bin_width: float = DEFAULT_BIN_WIDTH, max_bins: int = DEFAULT_MAX_BINS,
                 mask_threshold: Optional[float] = None, batch: int = 8, prefixes=None, **switches) -> List[dict]:
    """Every patient (and modality) of an image dataset (`data.ImageDatasets`) -> rows {'MRN': uid, feature: value}; written as a csv
    to `out_path` when given.  The uploads and kernels of `batch` patients are all enqueued before the first read-back of the batch.
    A dataset of two modalities prefixes its columns `t1_` / `t2_`.  `switches`: those of `extract` (`classes`, `glszm`, `mesh`,
    `log_sigma`, `log_bin_width`, `normalize`, `resample`, `shell_mm`), handed to it unchanged: the columns of the texture classes follow
    FEATURE_NAMES, the shells' follow all the others, and every block they add comes back in the batch's same stacked read-back; the
    pre-steps add nothing to it."""
    from .data import ingest
    dev = torch.device(device)
    rows = []
    patients = list(dataset.patients)
    for b0 in range(0, len(patients), max(1, int(batch))):
        chunk = patients[b0:b0 + max(1, int(batch))]
        raws = [_volumes_of(dataset, p) for p in chunk]
        up = [[(ingest.upload(s, dev), ingest.stage_mask(s, m, dev)) for s, m in vols] for vols in raws]
        maps = [[ingest.mask_index_map(s, m, getattr(dataset, "mask_resample", "auto")) for s, m in vols] for vols in up]
        res = [[extract(s, m, dev, bin_width, max_bins, index_map=t, threshold=mask_threshold, **switches) for (s, m), t in zip(vols, ts)]
               for vols, ts in zip(up, maps)]
        blocks = torch.stack([_stacked(r) for rs in res for r in rs]).cpu().numpy()      # the batch's one read-back
        k = 0
        for p, rs in zip(chunk, res):
            uid = dataset._uid_of(p)
            pre = prefixes if prefixes is not None else (("",) if len(rs) == 1 else ("t1_", "t2_"))
            row = {"MRN": uid}
            for r, px in zip(rs, pre):
                feats = _features_of_stacked(blocks[k], r, r.affine, f"patient {p} (uid {uid})")
                row.update({px + n: v for n, v in feats.items()})
                k += 1
            rows.append(row)
    if out_path is not None:
        write_csv(out_path, rows)
    return rows


def extract_modalities(datasets, device, bin_width: float = DEFAULT_BIN_WIDTH, max_bins: int = DEFAULT_MAX_BINS,
                       mask_threshold: Optional[float] = None, **switches) -> List[dict]:
    """`extract_tree` (with its `switches`) over one image dataset per modality: the columns of two modalities are prefixed `t1_` /
    `t2_` and their rows merged on `MRN`, in the first one's order, keeping the patients both have."""
    rows = None
    for ds, px in zip(datasets, ("t1_", "t2_") if len(datasets) == 2 else ("",)):
        part = extract_tree(ds, device, None, bin_width, max_bins, mask_threshold, prefixes=(px,), **switches)
        if rows is None:
            rows = part
        else:
            by = {r["MRN"]: r for r in part}
            rows = [dict(r, **{k: v for k, v in by[r["MRN"]].items() if k != "MRN"}) for r in rows if r["MRN"] in by]
    return rows


def write_csv(path, rows: List[dict]) -> None:
    cols = list(rows[0].keys()) if rows else ["MRN"] + list(FEATURE_NAMES)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for r in rows:
            w.writerow([r[c] if c == "MRN" else repr(float(r[c])) for c in cols])


def read_csv(path):
    """(columns, rows of strings) of a csv."""
    with open(path, newline="") as f:
        rd = csv.reader(f)
        cols = next(rd)
        return cols, [r for r in rd if r]


def add_extraction_arguments(ap, when: str = "") -> None:
    """The command-line switches of the extraction that main.py and this module's tool share; `Parser.radiomicsExtraction` resolves them
    against the config.  `when`: what the command line puts in front of the help texts of the switches that add columns or steps."""
    ap.add_argument("--mesh_shape", action="store_true", help=when + "append the 8 mesh-based shape columns (mesh volume, surface area, "
                    "sphericity, the diameters) to the extracted table; also switched on by the config's `Radiomics: mesh_shape: true`")
    ap.add_argument("--log_sigma", type=str, default=None, help=when + "Laplacian-of-Gaussian scales in mm, comma-separated (1,3): append the "
                    "log-sigma-<sigma>-mm-3D_* columns of the filtered scans; overrides the config's `Radiomics: log: sigma`")
    ap.add_argument("--log_bin_width", type=float, default=None, help="bin width of the filtered images; overrides the config's "
                    "`Radiomics: log: bin_width` (default: `Radiomics: bin_width`)")
    ap.add_argument("--normalize", action="store_true", help=when + "z-score the whole scan before the extraction "
                    "((v - mean) / sd * scale); also switched on by the config's `Radiomics: normalize`, or by either of the two values below")
    ap.add_argument("--normalize_scale", type=float, default=None, help="what the z-score is multiplied by; overrides `Radiomics: normalize: "
                    "scale` (default 100: with the default bin width of 25 PyRadiomics' scale of 1 would put every voxel into one bin)")
    ap.add_argument("--normalize_outliers", type=float, default=None, help="clamp the normalised values to +-K scale; overrides `Radiomics: "
                    "normalize: outliers` (default 0: no clamp)")
    ap.add_argument("--resample_spacing", type=str, default=None, help="resample scan and mask to this voxel spacing in mm before the "
                    "extraction, one number or three comma-separated (1,1,1; 0 keeps an axis); overrides `Radiomics: resample: spacing`")
    ap.add_argument("--shell_mm", type=str, default=None, help=when + "widths in mm of the peritumoural shells, comma-separated (5,10): append "
                    "the shell-<r>-mm_* columns of the tissue within r mm around the mask (never the shape classes); overrides the config's "
                    "`Radiomics: shell_mm`")


def tree_datasets(parser, directories, key_loc) -> list:
    """One image dataset per modality directory, read as the config's `Data:` section says (`mask_resample`, `format`, `mask_roi`)."""
    from .data.ImageDatasets import ImageDataset
    return [ImageDataset(d, key_loc, parser.maskResample()[0], format=parser.dataFormat(), mask_roi=parser.maskRoi()) for d in directories]


def build_arg_parser():
    ap = argparse.ArgumentParser(description="Extract radiomic features of every patient of an image tree on the device.")
    ap.add_argument("--image_loc", required=True)
    ap.add_argument("--key_loc", required=True)
    ap.add_argument("--config", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--modality", choices=("t1", "t2", "t1t2"), default="t1t2")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--classes", default=None, help="texture classes beside the 47 default columns: a comma-separated list of glrlm, gldm, "
                    "ngtdm, or 'all'; overrides the config's `Radiomics: classes`")
    ap.add_argument("--glszm", action="store_true", help="append the 16 size-zone (GLSZM) columns; also switched on by the config's "
                    "`Radiomics: glszm: true`")
    add_extraction_arguments(ap)
    return ap


def main(argv=None):
    a = build_arg_parser().parse_args(argv)
    import os
    from .parser.parser import Parser
    parser = Parser(a.config)
    data = parser.parseConfig().get("Data") or {}
    settings = parser.radiomicsExtraction(a)
    dirs = [os.path.join(a.image_loc, data.get(k, d)) for k, d in (("t1_path", "t1"), ("t2_path", "t2"))]
    dirs = [d for d, m in zip(dirs, ("t1", "t2")) if m in a.modality and os.path.isdir(d)]
    if not dirs:
        raise SystemExit(f"no modality directory under {a.image_loc}")
    rows = extract_modalities(tree_datasets(parser, dirs, a.key_loc), a.device, **settings)
    write_csv(a.out, rows)
    print(f"{len(rows)} patients, {len(rows[0]) - 1 if rows else 0} features -> {a.out}")


if __name__ == "__main__":
    main()
