"""Radiomic features of a (scan, mask) pair, extracted on the device: binding of `mmnn_radiomics` (csrc/radiomics.hip).

    extract(scan, mask, device)            enqueue one extraction; the result holds device tensors, nothing is read back
    finish(result, affine)                 one read-back -> {feature name: float}: adds TotalEnergy and the voxel-based shape features
    extract_tree(dataset, device, out)     every patient and modality of an image dataset -> a csv (`MRN`, then the features)
    python -m mmnn_sts_amd.radiomics --image_loc DIR --key_loc key.csv [--config c.yaml] --out radiomics.csv

Upstream reads such a csv (`Data: rad_loc`, data/RadiomicsDatasets.py) and leaves its extraction to PyRadiomics; here the table is built
from the very pair the image path ingests, through the same mask routes (NIfTI mask, resampled mask, DICOM mask series, RTSTRUCT, SEG:
`data.ingest.prepare_pair`).  The 47 columns carry PyRadiomics' names and definitions -- 18 first-order, 6 voxel-based shape, 23 GLCM --
in voxel index space (distance 1, no resampling, fixed `bin_width`).  Mesh-based shape features (surface area, sphericity, the
diameters) and the GLCM's MCC are out of scope.  What the numbers are pinned to is the numpy restatement in tests/_radiomics_ref.py.
"""
import argparse
import csv
import ctypes
import logging
import math
from dataclasses import dataclass
from typing import Dict, List, Optional

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
FEATURE_NAMES = tuple([f"original_firstorder_{n}" for n in FIRSTORDER] + [f"original_shape_{n}" for n in SHAPE]
                      + [f"original_glcm_{n}" for n in GLCM])
_logged_identity = False


@dataclass
class RadiomicsResult:
    """One extraction, still on the device.  `block`: the bytes of mmnn_radiomics_result; `hist` (max_bins,) and `glcm`
    (13, max_bins, max_bins) int32 views of the uint32 counts; `shape`, `affine`: the scan's grid."""
    block: torch.Tensor
    hist: torch.Tensor
    glcm: torch.Tensor
    workspace: torch.Tensor
    shape: tuple
    affine: Optional[np.ndarray]
    bin_width: float
    max_bins: int


def workspace_bytes(x: int, y: int, z: int, max_bins: int = DEFAULT_MAX_BINS) -> int:
    n = _lib.lib().mmnn_radiomics_workspace_bytes(int(x), int(y), int(z), int(max_bins))
    if n < 0:
        raise ValueError("mmnn_radiomics_workspace_bytes: " + _lib.last_error())
    return int(n)


def extract(scan, mask, device, bin_width: float = DEFAULT_BIN_WIDTH, max_bins: int = DEFAULT_MAX_BINS, index_map=None,
            threshold: Optional[float] = None, buffers: Optional[RadiomicsResult] = None) -> RadiomicsResult:
    """Enqueue the extraction of one (scan, mask) pair on the current stream of `device`.  `scan` / `mask`: whatever `ingest_volume`
    takes (host volumes are uploaded; a contour, SEG or other-grid mask is brought onto the scan's grid first, `index_map` and
    `threshold` as there).  `buffers`: a former result of the same extents and `max_bins` whose tensors are written again."""
    from .data import ingest
    dev = torch.device(device)
    scan, mask = ingest.prepare_pair(scan, mask, dev, index_map, threshold, what="radiomics")
    x, y, z = scan.shape
    max_bins = int(max_bins)
    nbytes = workspace_bytes(x, y, z, max_bins)
    if buffers is not None and (tuple(buffers.shape) != (x, y, z) or buffers.max_bins != max_bins or buffers.block.device != scan.data.device):
        raise ValueError(f"radiomics: buffers of extent {buffers.shape} / {buffers.max_bins} bins cannot take a scan of {(x, y, z)} / {max_bins}")
    dev = scan.data.device
    if buffers is None:
        block = torch.empty(_lib.RADIOMICS_RESULT_BYTES, dtype=torch.uint8, device=dev)
        hist = torch.empty(max_bins, dtype=torch.int32, device=dev)
        glcm = torch.empty((_lib.RADIOMICS_DIRECTIONS, max_bins, max_bins), dtype=torch.int32, device=dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        block, hist, glcm, ws = buffers.block, buffers.hist, buffers.glcm, buffers.workspace
    desc = _lib.RadiomicsDesc(x, y, z, scan.datatype, mask.datatype, float(scan.slope), float(scan.inter), float(mask.slope), float(mask.inter),
                              float(bin_width), max_bins)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mmnn_radiomics(ctypes.byref(desc), scan.data.data_ptr(), mask.data.data_ptr(), block.data_ptr(), hist.data_ptr(),
                                             glcm.data_ptr(), ws.data_ptr(), stream), "mmnn_radiomics")
    return RadiomicsResult(block, hist, glcm, ws, (x, y, z), scan.affine, float(bin_width), max_bins)


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


def features_of(fields: dict, affine, what: str = "radiomics") -> Dict[str, float]:
    """The host half of `finish`, from the unpacked block."""
    global _logged_identity
    if fields["empty"]:
        raise ConfigurationError(f"{what}: the mask selects no voxel of the scan")
    if fields["nonfinite"]:
        raise ConfigurationError(f"{what}: a NaN or infinite voxel value lies inside the mask")
    if fields["overflow"]:
        raise ConfigurationError(f"{what}: the values inside the mask span {fields['n_bins']} bins, more than max_bins: choose a larger "
                                 "bin_width (Radiomics: bin_width) or more bins (Radiomics: max_bins)")
    if affine is None:
        if not _logged_identity:
            logger.info("radiomics: a scan without an affine: shape features in voxel units (the identity)")
            _logged_identity = True
        linear = np.eye(3)
    else:
        linear = np.asarray(affine, dtype=np.float64)[:3, :3]
    out = {}
    fo = dict(zip(DEVICE_FIRSTORDER, (float(v) for v in fields["firstorder"])))
    shape = shape_features(fields["n"], fields["moments"], linear)
    fo["TotalEnergy"] = fo["Energy"] * abs(float(np.linalg.det(linear)))
    for n in FIRSTORDER:
        out[f"original_firstorder_{n}"] = fo[n]
    for n in SHAPE:
        out[f"original_shape_{n}"] = shape[n]
    for n, v in zip(GLCM, fields["glcm"]):
        out[f"original_glcm_{n}"] = float(v)
    return out


def finish(result: RadiomicsResult, affine="scan", what: str = "radiomics") -> Dict[str, float]:
    """One read-back of the result block -> {name: float} over FEATURE_NAMES.  `affine`: the scan's voxel index -> mm matrix (4x4 or
    its 3x3 linear part as the top-left block), None for the identity; the default takes the scan's own.  A flag raises
    ConfigurationError with the cause."""
    if isinstance(affine, str):
        affine = result.affine
    return features_of(unpack_block(result.block.cpu().numpy()), affine, what)


def _volumes_of(dataset, patient):
    return dataset._volumes(patient) if hasattr(dataset, "_volumes") else [dataset._load(patient)]


def extract_tree(dataset, device, out_path=None, bin_width: float = DEFAULT_BIN_WIDTH, max_bins: int = DEFAULT_MAX_BINS,
                 mask_threshold: Optional[float] = None, batch: int = 8, prefixes=None) -> List[dict]:
    """Every patient (and modality) of an image dataset (`data.ImageDatasets`) -> rows {'MRN': uid, feature: value}; written as a csv
    to `out_path` when given.  The uploads and kernels of `batch` patients are all enqueued before the first read-back of the batch.
    A dataset of two modalities prefixes its columns `t1_` / `t2_`."""
    from .data import ingest
    dev = torch.device(device)
    rows = []
    patients = list(dataset.patients)
    for b0 in range(0, len(patients), max(1, int(batch))):
        chunk = patients[b0:b0 + max(1, int(batch))]
        raws = [_volumes_of(dataset, p) for p in chunk]
        up = [[(ingest.upload(s, dev), ingest.stage_mask(s, m, dev)) for s, m in vols] for vols in raws]
        maps = [[ingest.mask_index_map(s, m, getattr(dataset, "mask_resample", "auto")) for s, m in vols] for vols in up]
        res = [[extract(s, m, dev, bin_width, max_bins, index_map=t, threshold=mask_threshold) for (s, m), t in zip(vols, ts)]
               for vols, ts in zip(up, maps)]
        blocks = torch.stack([r.block for rs in res for r in rs]).cpu().numpy()          # the batch's one read-back
        k = 0
        for p, rs in zip(chunk, res):
            uid = dataset._uid_of(p)
            pre = prefixes if prefixes is not None else (("",) if len(rs) == 1 else ("t1_", "t2_"))
            row = {"MRN": uid}
            for r, px in zip(rs, pre):
                feats = features_of(unpack_block(blocks[k]), r.affine, f"patient {p} (uid {uid})")
                row.update({px + n: v for n, v in feats.items()})
                k += 1
            rows.append(row)
    if out_path is not None:
        write_csv(out_path, rows)
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


def main(argv=None):
    ap = argparse.ArgumentParser(description="Extract radiomic features of every patient of an image tree on the device.")
    ap.add_argument("--image_loc", required=True)
    ap.add_argument("--key_loc", required=True)
    ap.add_argument("--config", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--modality", choices=("t1", "t2", "t1t2"), default="t1t2")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    import os
    from .data.ImageDatasets import ImageDataset
    from .parser.parser import Parser
    config = Parser(a.config).parseConfig()
    data, rad = dict(config.get("Data") or {}), dict(config.get("Radiomics") or {})
    dirs = [os.path.join(a.image_loc, data.get(k, d)) for k, d in (("t1_path", "t1"), ("t2_path", "t2"))]
    dirs = [d for d, m in zip(dirs, ("t1", "t2")) if m in a.modality and os.path.isdir(d)]
    if not dirs:
        raise SystemExit(f"no modality directory under {a.image_loc}")
    sets = [ImageDataset(d, a.key_loc, str(data.get("mask_resample", "auto")).lower(), format=data.get("format"), mask_roi=data.get("mask_roi"))
            for d in dirs]
    rows = None
    for ds, px in zip(sets, ("t1_", "t2_") if len(sets) == 2 else ("",)):
        part = extract_tree(ds, a.device, None, float(rad.get("bin_width", DEFAULT_BIN_WIDTH)), int(rad.get("max_bins", DEFAULT_MAX_BINS)),
                            data.get("mask_threshold"), prefixes=(px,))
        if rows is None:
            rows = part
        else:
            by = {r["MRN"]: r for r in part}
            rows = [dict(r, **{k: v for k, v in by[r["MRN"]].items() if k != "MRN"}) for r in rows if r["MRN"] in by]
    write_csv(a.out, rows)
    print(f"{len(rows)} patients, {len(rows[0]) - 1 if rows else 0} features -> {a.out}")


if __name__ == "__main__":
    main()
