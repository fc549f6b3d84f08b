"""A seeded synthetic patient tree in the layout the NIfTI datasets read (`mmnn_sts_amd.data.ImageDatasets`), for the tests, the timing
tool and a first run of `main.py --image_loc` before it is pointed at patients.

    <root>/images/t1/SYN-0007-t1-a/scan_t1.nii.gz, mask.nii.gz       int16 scan (slope 0.25, inter -12.5), uint8 ellipsoid mask
    <root>/images/t2/SYN-0007-t2-a/scan_t2.nii.gz, mask.nii.gz
    <root>/key.csv                                                    Anon MRN, MRN
    <root>/clinical.csv                                               uid, predictors, event{i}, duration{i} (main.py: write_synthetic_csv)
    <root>/train_uids.txt, <root>/val_uids.txt                        one uid per line

Extents are ragged (drawn per patient and shared by its modalities); every mask has at least one interior empty slice along each axis.
With `mask_grid="own"` every mask is written on a grid of its own -- other extents, coarser spacing, a small rotation and an offset
against the scan, whose affine is not the identity either -- as a contour drawn on another series arrives; the datasets then resample
it into the scan's grid on the device.

    python -m mmnn_sts_amd.data.synth_nifti /tmp/syn --patients 8 [--mask_grid own]
"""
import argparse
import os

import numpy as np

from . import nifti
from .constants import NUM_CLASSES

SCAN_SLOPE, SCAN_INTER = 0.25, -12.5


def ellipsoid_mask(shape, rng, holes=True):
    """uint8 ellipsoid somewhere inside `shape`; with `holes`, one interior slice per axis is cleared (so it is empty after masking)."""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    centre = [n * (0.5 + 0.1 * (rng.random() - 0.5)) for n in shape]
    radius = [max(2.0, n * (0.25 + 0.15 * rng.random())) for n in shape]
    m = (sum(((g - c) / r) ** 2 for g, c, r in zip(grids, centre, radius)) <= 1.0).astype(np.uint8)
    if holes:
        for axis in range(3):
            kept = np.flatnonzero(m.any(axis=tuple(a for a in range(3) if a != axis)))
            if len(kept) >= 3:
                sl = [slice(None)] * 3
                sl[axis] = int(kept[1 + rng.integers(0, len(kept) - 2)])
                m[tuple(sl)] = 0
    return m


def synth_scan(shape, rng):
    """int16 voxels: a smooth ramp plus noise, strictly positive after `raw * SCAN_SLOPE + SCAN_INTER`."""
    ramp = sum(np.linspace(0.0, 200.0, n).reshape([-1 if a == k else 1 for a in range(3)]) for k, n in enumerate(shape))
    return (100.0 + ramp + rng.integers(0, 400, shape)).astype(np.int16)


def _rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _affine(linear, offset):
    a = np.eye(4)
    a[:3, :3], a[:3, 3] = linear, offset
    return a


def own_grid(mask, rng):
    """(mask on a grid of its own, scan affine, mask affine): the scan grid gets 0.9 x 0.9 x 3 mm voxels, a small rotation and an offset;
    the mask grid is coarser by 1.15-1.45 per axis, rotated a little further about the volume's centre, and its extents differ from
    the scan's on every axis.  The mask's voxels are the scan-grid mask at the nearest scan voxel (0 outside)."""
    shape = np.asarray(mask.shape)
    scan_affine = _affine(_rot_z(rng.uniform(-0.08, 0.08)) @ np.diag([0.9, 0.9, 3.0]), rng.uniform(-80.0, 80.0, 3))
    factor = rng.uniform(1.15, 1.45, 3)
    own = np.ceil(shape / factor).astype(int) + 1
    own += own == shape
    # mask index -> scan index: about the two centres, a rotation in the (x, y) plane and the coarser spacing
    lin = _rot_z(rng.uniform(-0.06, 0.06)) @ np.diag(factor)
    to_scan = _affine(lin, (shape - 1) / 2.0 + rng.uniform(-0.4, 0.4, 3) - lin @ ((own - 1) / 2.0))
    idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in own], indexing="ij"), axis=-1)
    at = np.rint(idx @ to_scan[:3, :3].T + to_scan[:3, 3]).astype(int)
    inside = ((at >= 0) & (at < shape)).all(axis=-1)
    at = np.clip(at, 0, shape - 1)
    out = np.where(inside, mask[at[..., 0], at[..., 1], at[..., 2]], 0).astype(mask.dtype)
    return out, scan_affine, scan_affine @ to_scan


def write_tree(root, n_patients=6, seed=0, predictors=None, extent=((24, 40), (24, 40), (10, 20)), modalities=("t1", "t2"),
               empty_mask_uids=(), val_fraction=0.34, gz=True, mask_grid="same"):
    """Write the tree; returns {'image_loc', 't1_path', 't2_path', 'key_loc', 'data_loc', 'train_uids', 'val_uids', 'uids'}.
    `mask_grid`: 'same' (mask and scan share one grid and the identity affine) or 'own' (see `own_grid`; its draws come from a
    generator of their own, so scans, masks on the scan grid and labels are those of 'same')."""
    if mask_grid not in ("same", "own"):
        raise ValueError(f"mask_grid {mask_grid!r} is neither 'same' nor 'own'")
    root = str(root)
    rng = np.random.default_rng(seed)
    grid_rng = np.random.default_rng([int(seed), 1])
    predictors = [f"predictor{i}" for i in range(32)] if predictors is None else list(predictors)
    uids = [1000 + 7 * i for i in range(n_patients)]
    image_loc = os.path.join(root, "images")
    ext = ".nii.gz" if gz else ".nii"
    for i, uid in enumerate(uids):
        shape = tuple(int(rng.integers(lo, hi + 1)) for lo, hi in extent)
        for mod in modalities:
            d = os.path.join(image_loc, mod, f"SYN-{i:04d}-{mod}-a")
            os.makedirs(d, exist_ok=True)
            mask = ellipsoid_mask(shape, rng)
            if uid in empty_mask_uids:
                mask[:] = 0
            scan_affine = mask_affine = None
            if mask_grid == "own":
                mask, scan_affine, mask_affine = own_grid(mask, grid_rng)
            nifti.write(os.path.join(d, f"scan_{mod}{ext}"), synth_scan(shape, rng), SCAN_SLOPE, SCAN_INTER, affine=scan_affine)
            nifti.write(os.path.join(d, f"mask{ext}"), mask, affine=mask_affine)
    key = os.path.join(root, "key.csv")
    with open(key, "w") as f:
        f.write("Anon MRN,MRN\n")
        for i, uid in enumerate(uids):
            f.write(f"SYN-{i:04d},{uid}\n")
    cols = ["uid"] + predictors + [f"event{i}" for i in range(NUM_CLASSES)] + [f"duration{i}" for i in range(NUM_CLASSES)]
    events = (rng.random((n_patients, NUM_CLASSES)) < 0.6).astype(np.float64)
    events[0, :] = 1.0                                   # at least one observed event per target
    rows = np.concatenate([np.asarray(uids, dtype=np.float64)[:, None], rng.standard_normal((n_patients, len(predictors))), events,
                           rng.integers(1, 3000, (n_patients, NUM_CLASSES)).astype(np.float64)], axis=1)
    data = os.path.join(root, "clinical.csv")
    np.savetxt(data, rows, delimiter=",", header=",".join(cols), comments="", fmt="%.9g")
    n_val = max(1, int(round(n_patients * val_fraction)))
    order = [uids[i] for i in rng.permutation(n_patients)]
    lists = {"train_uids": order[n_val:], "val_uids": order[:n_val]}
    out = {"image_loc": image_loc, "t1_path": "t1", "t2_path": "t2", "key_loc": key, "data_loc": data, "uids": uids}
    for name, members in lists.items():
        out[name] = os.path.join(root, name + ".txt")
        with open(out[name], "w") as f:
            f.write("".join(f"{u}\n" for u in members))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("root")
    ap.add_argument("--patients", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mask_grid", choices=("same", "own"), default="same", help="own: every mask on a grid of its own, to be resampled")
    a = ap.parse_args()
    for k, v in write_tree(a.root, a.patients, a.seed, mask_grid=a.mask_grid).items():
        print(f"{k}: {v}")
