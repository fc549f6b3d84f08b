#!/usr/bin/env python
"""CLI of the fusion path with the reference's flag surface (main.py:897-1022 of DigITs-AIML/MMNN_STS).

    python main.py --preop --classification                       # BASELINE configs[0] (tabular MLP from a 32 x 64 csv)
    python main.py --images --survival                            # configs[1] (unimodal DenseNet, t1)
    python main.py --images --preop --survival --blend            # configs[2] (T1+T2+tabular, GradientBlender)
    python main.py --inference --images --preop --survival        # configs[4] (Grad-CAM attention maps)

Training loops = main.py:385-601 (survival) and :125-327 (classification) restated.  Survival: micro-batches, gradients
accumulated until SUPER_BATCH_SIZE (64) patients were seen, SGD-Nesterov + OneCycleLR stepped per super-batch, GradientBlender
weight update every `--blend_update_interval` epochs, C-index per epoch, best model (by the un-weighted fused-head loss of the
last validation batch, as upstream :525,573) saved as best_surv_model.pth.  Classification: pos-weighted BCE on logits, one
optimizer step per batch, F1 per epoch, best model by mean validation F1 saved as model.pth, optional GradientBlender.
Deviations from the reference, all listed in SURVEY Appendix A: the published script cannot be imported (Q1) -- its third assert
is dropped and CLASS_FREQUENCIES comes from the config; the validation loop moves `val_images` (Q10); the blender lives on the
loss device (Q4); logging syncs once per epoch, not per micro-batch; `--preop` alone builds the standalone MLP (Q12).
What each flag beyond upstream's does is in its help text and in INTEGRATION.md.  `resolve_settings` checks the command line against the
config once and `build_data_source` picks the datasets: patient directories (`--image_loc`), a radiomics table (`--radiomics`), a clinical
csv, or synthetic patients.  There is no CPU compute path: every model runs on the MI355X through the HIP library (configs[0]'s "CPU" is
upstream's device).  With WORLD_SIZE > 1 (torch.distributed.run) patients are sharded over the ranks and gradients SUM-all-reduced (RCCL).
"""
import argparse
import contextlib
import logging
import os
import sys
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from mmnn_sts_amd import distributed as D  # noqa: E402
from mmnn_sts_amd.data.constants import CLASSIFICATION_THRESHOLD, NUM_BOOTSTRAP_ITERATIONS, NUM_CLASSES, SUPER_BATCH_SIZE  # noqa: E402
from mmnn_sts_amd.losses.GradientBlender import GradientBlender  # noqa: E402
from mmnn_sts_amd.losses.losses import BCEWithLogitsLoss, CoxPH  # noqa: E402
from mmnn_sts_amd.optim import FusedSGD  # noqa: E402
from mmnn_sts_amd.exceptions.exceptions import ConfigurationError  # noqa: E402
from mmnn_sts_amd.parser.parser import Parser  # noqa: E402
from mmnn_sts_amd.utils.utils import add_gradcam, add_occlusion, criterion, loadWeights, surv_criterion  # noqa: E402

logging.basicConfig(level=logging.INFO, format="%(message)s")
logger = logging.getLogger("mmnn_sts_amd")


def str_to_bool(arg):
    if arg.lower() == 'false':
        return False
    if arg.lower() == 'true':
        return True
    raise ValueError('Unexpected value for boolean conversion: {}'.format(arg))


# ---- epoch-level bookkeeping (host logic, unit-tested on CPU) --------------------------------------------------------------
def concordance_index(event_times, predicted_scores, event_observed):
    """Harrell's C as `lifelines.utils.concordance_index(event_times, predicted_scores, event_observed)` computes it (main.py:33,
    122; lifelines is not vendored => restated from its published algorithm, parity unpinned).  An ordered pair (a, b) is
    admissible when a is an observed event and b outlived a: t_b > t_a, or t_b == t_a with b censored (lifelines handles the
    deaths of a time before its censored cases).  It is concordant when a also has the lower score, half-credit for equal scores.
    NaN when no pair is admissible (lifelines raises ZeroDivisionError there)."""
    t, s, e = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (event_times, predicted_scores, event_observed))
    died = e > 0
    later = t[None, :] > t[:, None]
    same_time_censored = (t[None, :] == t[:, None]) & ~died[None, :]
    admissible = died[:, None] & (later | same_time_censored)
    n = int(admissible.sum())
    if n == 0:
        return float("nan")
    lower = s[:, None] < s[None, :]
    equal = s[:, None] == s[None, :]
    return float((lower & admissible).sum() + 0.5 * (equal & admissible).sum()) / n


def getCIndices(preds, events, durations):
    """main.py:106-123: one C-index per survival target."""
    return [concordance_index(durations[:, i], preds[:, i], events[:, i]) for i in range(NUM_CLASSES)]


def getF1Score(tps, fps, fns):
    """main.py:97-104."""
    return [float(tps[i] / (tps[i] + 0.5 * (fns[i] + fps[i]))) for i in range(NUM_CLASSES)]


def super_batch_interval(batch_size: int, world: int = 1) -> int:
    """Micro-batches per optimizer step (main.py:403): gradients are summed until SUPER_BATCH_SIZE patients were seen -- by all
    ranks together when the patients are sharded over `world` ranks."""
    return max(1, SUPER_BATCH_SIZE // (batch_size * world))


def optimizer_steps_per_epoch(n_batches: int, interval: int) -> int:
    """Optimizer / scheduler steps of one epoch: every `interval`-th micro-batch plus the ragged tail.  Equals upstream's
    ceil(len(train_dataset) / SUPER_BATCH_SIZE) (main.py:404-407) whenever the batch size divides SUPER_BATCH_SIZE."""
    return max(1, -(-n_batches // interval))


def is_step_boundary(i: int, n_batches: int, interval: int) -> bool:
    """main.py:478: step on every `interval`-th micro-batch and on the last one of the epoch."""
    return (i + 1) % interval == 0 or i == n_batches - 1


def blender_update_due(epoch: int, interval: int) -> bool:
    """main.py:584: epochs are 0-based here as upstream."""
    return (epoch + 1) % interval == 0


def gather_rows(t: torch.Tensor, dim: int, world: int) -> torch.Tensor:
    """Concatenate a per-rank tensor over all ranks along `dim` (identity for one rank): the blender's epoch-level losses must be
    computed on ALL patients so that every rank derives the same head weights."""
    if world == 1:
        return t
    parts = [torch.empty_like(t) for _ in range(world)]
    torch.distributed.all_gather(parts, t.contiguous())
    return torch.cat(parts, dim=dim)


def bootstrap_c_indices(preds, events, durations, iterations: int = NUM_BOOTSTRAP_ITERATIONS, seed: int = 0):
    """main.py:767-768,857-887 (`--bootstrap`): C-indices of `iterations` resamples (with replacement, same size) of the evaluated
    patients -> (per-target means, per-target standard deviations, number of usable resamples).  Upstream re-runs the model over every
    resampled uid list; in eval mode with batch size 1 a patient's prediction does not depend on its neighbours, so resampling the
    PREDICTIONS of one pass gives the same numbers at 1/50th of the device work.  A resample without any admissible pair is skipped
    (upstream: `except ZeroDivisionError: continue`, :857-858)."""
    preds, events, durations = (np.asarray(t) for t in (preds, events, durations))
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(iterations):
        idx = rng.integers(0, len(preds), len(preds))
        c = getCIndices(preds[idx], events[idx], durations[idx])
        if not np.any(np.isnan(c)):
            rows.append(c)
    if not rows:
        return [float("nan")] * NUM_CLASSES, [float("nan")] * NUM_CLASSES, 0
    arr = np.asarray(rows)
    return arr.mean(axis=0).tolist(), arr.std(axis=0).tolist(), len(rows)


# ---- data plumbing -----------------------------------------------------------------------------------------------------------
class SyntheticPatients(torch.utils.data.Dataset):
    """Stand-in for MultiModalSurvivalDataset (data/MultiModalDatasets.py:8-86): {'image','clinical'}, events, durations."""

    def __init__(self, n, in_channels, size, n_clinical, multimodal, images, seed):
        g = torch.Generator().manual_seed(seed)
        self.images = torch.randn((n, in_channels, size, size, size), generator=g) if images else None
        self.clinical = torch.randn((n, n_clinical), generator=g)
        self.events = (torch.rand((n, NUM_CLASSES), generator=g) < 0.6).long()
        self.durations = torch.randint(1, 3000, (n, NUM_CLASSES), generator=g)
        self.multimodal = multimodal

    def __len__(self):
        return self.clinical.shape[0]

    def __getitem__(self, i):
        if self.multimodal:
            x = {"image": self.images[i], "clinical": self.clinical[i]}
        else:
            x = self.images[i] if self.images is not None else self.clinical[i]
        return x, self.events[i], self.durations[i]


def write_synthetic_csv(path, n_patients, predictors, seed):
    """The tabular plumbing of BASELINE configs[0]: one row per patient -- uid, the predictor columns, then per target an event
    flag and a duration -- as data/ClinicalDatasets.py:6-89 reads it from its csv."""
    g = np.random.default_rng(seed)
    cols = ["uid"] + list(predictors) + [f"event{i}" for i in range(NUM_CLASSES)] + [f"duration{i}" for i in range(NUM_CLASSES)]
    rows = np.concatenate([np.arange(n_patients)[:, None], g.standard_normal((n_patients, len(predictors))),
                           (g.random((n_patients, NUM_CLASSES)) < 0.6).astype(np.float64),
                           g.integers(1, 3000, (n_patients, NUM_CLASSES)).astype(np.float64)], axis=1)
    np.savetxt(path, rows, delimiter=",", header=",".join(cols), comments="", fmt="%.9g")
    return path


class ClinicalCsvDataset(torch.utils.data.Dataset):
    """(features, events, durations) per patient from a csv written by `write_synthetic_csv` / shaped like it."""

    def __init__(self, path, predictors):
        with open(path) as f:
            header = f.readline().strip().split(",")
        table = np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)
        col = {name: i for i, name in enumerate(header)}
        missing = [p for p in predictors if p not in col]
        if missing:
            raise ValueError(f"csv {path} lacks predictor columns {missing[:4]}...")
        self.clinical = torch.from_numpy(table[:, [col[p] for p in predictors]]).float()
        self.events = torch.from_numpy(table[:, [col[f"event{i}"] for i in range(NUM_CLASSES)]]).long()
        self.durations = torch.from_numpy(table[:, [col[f"duration{i}"] for i in range(NUM_CLASSES)]]).long()

    def __len__(self):
        return self.clinical.shape[0]

    def __getitem__(self, i):
        return self.clinical[i], self.events[i], self.durations[i]


def collate(batch):
    xs, ev, du = zip(*batch)
    if isinstance(xs[0], dict):
        x = {k: torch.stack([b[k] for b in xs]).float() for k in xs[0]}
    else:
        x = torch.stack(xs).float()
    return x, torch.stack(ev), torch.stack(du)


def to_device(x, device):
    return {k: v.to(device) for k, v in x.items()} if isinstance(x, dict) else x.to(device)


NO_DEVICE = "mmnn_sts_amd runs on the MI355X only (no CPU path)"
DEFAULT_CACHE_GB = 16.0                      # a setting, not a measurement: about a twentieth of the card's 288 GB
# the synthetic sets: their seeds (every rank draws its own training patients, at TRAIN_SEED + rank) and, for `--synthetic_patients n`,
# their patient counts
TRAIN_SEED, VAL_SEED, EVAL_SEED = 1000, 7, 99


def synthetic_counts(n, classification):
    """(train, validation, evaluation) patients: the classification loop wants 4 of each at least, the survival loop 2 to validate on."""
    return (max(4, n), max(4, n // 4), max(2, n // 4)) if classification else (n, max(2, n // 4), max(2, n // 4))


@dataclass
class DataSource:
    """What the loops consume.  `ingest`: the device ingest of patient directories, which then is the loaders' collate function;
    `cache`: the volume cache behind it, sized for `cache_patients`.  `evaluation` is what `--inference` runs over."""
    train: Optional[torch.utils.data.Dataset] = None
    val: Optional[torch.utils.data.Dataset] = None
    evaluation: Optional[torch.utils.data.Dataset] = None
    ingest: Optional[Callable] = None
    train_tf: Optional[Callable] = None
    val_tf: Optional[Callable] = None
    cache: Optional[object] = None
    cache_patients: int = 0

    @property
    def collate(self):
        return self.ingest or collate


def report_empty_masks(ingest):
    """`--image_loc`: patients whose mask left nothing of a scan (the ingest wrote zeros for them; upstream crashes there) are named once
    and the run ends non-zero.  Reads the extents of every batch collated since the last call: call it where the epoch has synchronised."""
    empty = ingest.take_empty() if ingest is not None else []
    if empty:
        logger.error("empty mask: nothing of the scan is left after masking for patient uid(s) %s", ", ".join(str(u) for u in empty))
        raise SystemExit(f"empty mask for patient uid(s) {empty}: fix or remove these patients")


def log_volume_cache(data, rank):
    """`--cache_volumes`: one line per epoch -- what the cache holds, what it served in this epoch, and the files the datasets read in it."""
    if data.cache is None:
        return
    from mmnn_sts_amd.data.ImageDatasets import ImageDataset
    hits, misses, overflow = data.cache.table.take_counters()
    files, ImageDataset.files_read = ImageDataset.files_read, 0
    if rank == 0:
        logger.info("volume cache: %d of %d patients cached, %.1f MB held; this epoch: %d hits, %d misses, %d overflow, %d files read",
                    data.cache.table.n_filled, data.cache_patients, data.cache.bytes_held / 1e6, hits, misses, overflow, files)


def split_uids(uids, args, seed):
    """(train, val) uids: `--train_uid_location` / `--val_uid_location` when both files exist, else a seeded 80 / 20 split of the sorted uids."""
    from mmnn_sts_amd.utils.utils import loadUIDs
    if os.path.exists(args.train_uid_location) and os.path.exists(args.val_uid_location):
        return loadUIDs(args.train_uid_location), loadUIDs(args.val_uid_location)
    uids = sorted(uids)
    order = np.random.default_rng(seed).permutation(len(uids))
    n_val = min(max(1, round(0.2 * len(uids))), len(uids) - 1)
    return sorted(uids[i] for i in order[n_val:]), sorted(uids[i] for i in order[:n_val])


def scale_radiomics(parser, args, train_uids, rank):
    """`Radiomics: standardize`: z-score the radiomic columns with the training uids' mean / std, written to
    <output_path>/radiomics_scaler.csv; `--inference` reads that file back."""
    from mmnn_sts_amd.data.RadiomicsDatasets import SCALER_FILE
    if not parser.radiomicsConfig()["standardize"]:
        return
    ds, path = parser.radiomics_dataset, os.path.join(args.output_path, SCALER_FILE)
    if args.inference:
        if not os.path.exists(path):
            raise SystemExit(f"--inference --radiomics reads the scaler the training run wrote: {path} is missing (same --output_path, or "
                             "`Radiomics: standardize: false`)")
        ds.load_scaler(path)
        return
    ds.fit_scaler(train_uids)
    if rank == 0:
        os.makedirs(args.output_path, exist_ok=True)
        ds.save_scaler(path)


def tree_data_source(data, parser, args, device, rank, world):
    """`--image_loc`: upstream's datasets (parser.getDatasets) over the local patient tree, cut into the train and validation uids; the
    loaders' collate function becomes the device ingest, behind a volume cache with `--cache_volumes`."""
    from mmnn_sts_amd.data.ImageDatasets import ImageDatasetByUIDs
    full = parser.getDatasets(args, parser.getImagePath())
    train_uids, val_uids = split_uids(full.uids, args, args.seed)
    if args.radiomics:
        scale_radiomics(parser, args, train_uids, rank)
    by_uids, extras = ImageDatasetByUIDs, {}
    if args.cache_volumes:
        # one cache per process: this rank's training shard and the validation set, which every rank evaluates
        from mmnn_sts_amd.data.cache import CachedByUIDs, VolumeCache, capacity_for
        data.cache_patients = len(set(train_uids[rank::world]) | set(val_uids))
        data.cache = VolumeCache(device, args.in_channels, args.image_size,
                                 capacity_for(int(args.cache_gb * 2 ** 30), args.in_channels, args.image_size, data.cache_patients))
        by_uids = lambda dataset, uids: CachedByUIDs(dataset, uids, data.cache)
        extras["cache"] = data.cache
        if rank == 0:
            logger.info("volume cache: room for %d of %d patients (%d x %d^3 fp32 each) in %g GB", data.cache.capacity, data.cache_patients,
                        args.in_channels, args.image_size, args.cache_gb)
    if args.mask_margin_mm is not None:
        extras["mask_margin_mm"] = args.mask_margin_mm
    # `getDatasets` above has left the tree's layout on the parser (`image_layout`), which `maskResample()`'s default threshold depends
    # on (128 behind DICOM scans): the ingest is built behind it, here and nowhere else
    from mmnn_sts_amd.data.ingest import IngestCollate
    data.ingest = IngestCollate(device, *parser.maskResample(), keep_workspaces=args.scan_space, size=args.image_size, **extras)
    data.train, data.val = by_uids(full, train_uids[rank::world]), by_uids(full, val_uids)


def build_data_source(args, parser, rank=0, world=1, device=None) -> DataSource:
    """The datasets of the run, their collate function, the `--transforms` pipelines and the volume cache.  Only patient directories
    (`--image_loc`) need `device`, for their ingest.  `--inference` evaluates the validation uids of a tree or table, `--data_loc`
    (else the validation csv) of a clinical csv, and synthetic image patients of their own seed."""
    data = DataSource()
    if args.transforms:
        from mmnn_sts_amd.transforms import pipelines
        data.train_tf, data.val_tf = pipelines(args.image_size)
    if args.radiomics and not args.images:
        # the predictor table (radiomic columns, behind the clinical ones with --preop / --postop) cut into the train and validation uids
        from mmnn_sts_amd.data.RadiomicsDatasets import TableByUIDs
        full = parser.getDatasets(args)
        known = set(full.uids)
        train_uids, val_uids = ([u for u in uids if u in known] for uids in split_uids(full.uids, args, args.seed))
        scale_radiomics(parser, args, train_uids, rank)
        data.train, data.val = TableByUIDs(full, train_uids[rank::world]), TableByUIDs(full, val_uids)
    elif not args.images:
        # tabular-only: patients travel through a csv, as upstream's clinical datasets do (at the classification loop's counts)
        predictors = parser.predictors(args)
        os.makedirs(args.output_path, exist_ok=True)
        n_train, n_val, _ = synthetic_counts(args.synthetic_patients, True)
        train_csv = args.data_loc or write_synthetic_csv(os.path.join(args.output_path, f"synthetic_train_rank{rank}.csv"), n_train, predictors,
                                                         TRAIN_SEED + rank)
        val_csv = write_synthetic_csv(os.path.join(args.output_path, f"synthetic_val_rank{rank}.csv"), n_val, predictors, VAL_SEED)
        data.train, data.val = ClinicalCsvDataset(train_csv, predictors), ClinicalCsvDataset(val_csv, predictors)
        data.evaluation = ClinicalCsvDataset(args.data_loc or val_csv, predictors)        # --inference --data_loc x.csv evaluates THAT file
    elif args.use_nifti:
        tree_data_source(data, parser, args, device, rank, world)
    elif args.data_loc:
        raise SystemExit("clinical csv + image loaders need --image_loc (NIfTI patient directories) and --key_loc; run without --data_loc for synthetic patients")
    else:
        n_train, n_val, n_eval = synthetic_counts(args.synthetic_patients, args.classification)
        n_clinical = len(parser.predictors(args))
        patients = lambda n, seed: SyntheticPatients(n, args.in_channels, args.synthetic_size, n_clinical, args.multimodal, True, seed)
        if args.inference:
            data.evaluation = patients(n_eval, EVAL_SEED)
        else:
            data.train, data.val = patients(n_train, TRAIN_SEED + rank), patients(n_val, VAL_SEED)
    if data.evaluation is None:
        data.evaluation = data.val
    return data


def extract_radiomics_if_needed(parser, args):
    """`--radiomics` without `--rad_loc`: every patient (and modality) of the image tree -> <output_path>/radiomics_features.csv on the
    device, which then is the run's `rad_loc`."""
    data = parser.config["Data"]
    if data.get("rad_loc"):
        return
    from mmnn_sts_amd import radiomics
    if not torch.cuda.is_available():
        raise SystemExit(NO_DEVICE)
    settings = parser.radiomicsExtraction(args)
    paths = parser.getImagePath()
    sets = radiomics.tree_datasets(parser, paths if isinstance(paths, tuple) else (paths,), parser._data("key_loc"))
    rows = radiomics.extract_modalities(sets, torch.device("cuda", 0), **settings)
    os.makedirs(args.output_path, exist_ok=True)
    out = os.path.join(args.output_path, "radiomics_features.csv")
    radiomics.write_csv(out, rows)
    logger.info("radiomic features of %d patients -> %s", len(rows), out)
    data["rad_loc"] = out


def patient_folder(output_path, uid):
    """Upstream's per-patient folder (main.py:829-845), which the three exporters below write into."""
    return os.path.join(output_path, "attention_maps", f"_patient_{uid}")


def export_patient_nifti(d, image, att, preds):
    """Into the patient's folder `d`: {t1image,t2image,att_map}.nii.gz + preds.txt (main.py:829-845).  The volumes are written at the
    extent they have: S^3 under `--image_size S`."""
    from mmnn_sts_amd.data import nifti
    os.makedirs(d, exist_ok=True)
    for c, name in zip(range(image.shape[0]), ("t1image", "t2image")):
        nifti.write(os.path.join(d, name + ".nii.gz"), image[c].cpu().numpy().astype(np.float32))
    nifti.write(os.path.join(d, "att_map.nii.gz"), att.cpu().numpy().astype(np.float32))
    with open(os.path.join(d, "preds.txt"), "w") as f:
        f.write("".join(f"{float(v)!r}\n" for v in preds.reshape(-1)))


def export_occlusion_nifti(d, maps):
    """`--occlusion --image_loc`: occ_map_class{k}.nii.gz per output in the patient's folder `d`, beside att_map.nii.gz."""
    from mmnn_sts_amd.data import nifti
    os.makedirs(d, exist_ok=True)
    maps = maps.cpu().numpy().astype(np.float32)
    for k in range(maps.shape[0]):
        nifti.write(os.path.join(d, f"occ_map_class{k}.nii.gz"), maps[k])


def export_scan_space_maps(d, maps, volumes, prefix="att_map"):
    """`--scan_space`: every class's attention map on the voxel grid of every scan of the patient, into the patient's folder `d` as
    att_map_class{k}_on_{t1,t2}.nii.gz (att_map_class{k}_on_scan.nii.gz for a single modality; `prefix` replaces "att_map": the
    occlusion maps are written as occ_map_class{k}_on_*), written with the scan's affine so that a
    viewer lays it over the scan.  `maps`: (classes, S, S, S) on the device, in the model's space (S: `--image_size`, 64 by default); `volumes`: the patient's
    `KeptVolume` per modality.  The ingest's own kept slices are inverted on the device (`maps_to_scan`); dropped slices are 0."""
    from mmnn_sts_amd.data import nifti
    from mmnn_sts_amd.data.ingest import maps_to_scan
    os.makedirs(d, exist_ok=True)
    names = ("t1", "t2") if len(volumes) == 2 else ("scan",)
    for name, vol in zip(names, volumes):
        on_scan = maps_to_scan(maps, vol.shape, vol.workspace).cpu().numpy()           # (classes, z, y, x)
        for k in range(on_scan.shape[0]):
            nifti.write(os.path.join(d, f"{prefix}_class{k}_on_{name}.nii.gz"), on_scan[k].transpose(2, 1, 0), affine=vol.affine)


def apply_transforms(x, tf):
    """`--transforms`: upstream's train / val transforms (main.py:64-92) on the device batch -- the image itself for image-only runs,
    x['image'] for multimodal ones.  None: no transforms."""
    if tf is None:
        return x
    if isinstance(x, dict):
        return dict(x, image=tf(x["image"]))
    return tf(x)


def device_batches(batches, device, tf, targets=2):
    """Each (input, events, durations) of `batches` with the input on the device and through this phase's transforms `tf`, and the first
    `targets` of the other two on the device as well (the classification loops read the events alone; inference keeps both on the host)."""
    for x, ev, du in batches:
        x = to_device(x, device)
        if targets >= 1:
            ev = ev.to(device)
        if targets >= 2:
            du = du.to(device)
        yield apply_transforms(x, tf), ev, du


def end_of_epoch(data, rank, blender=None, blender_inputs=None):
    """Where an epoch has synchronised: the empty masks it met, the cache's line and, when `blender` is given (its update is due), the
    new head weights from `blender_inputs()`."""
    report_empty_masks(data.ingest)
    log_volume_cache(data, rank)
    if blender is not None:
        blender.updateWeights(*blender_inputs())
        if rank == 0:
            logger.info('Completed updating gradient blender weights - new weights : {}'.format(blender.weights))


# ---- survival (main.py:385-601) ----------------------------------------------------------------------------------------------
def train_survival(model, data, args, device, rank, world):
    train_ds, val_ds = data.train, data.val
    loader = torch.utils.data.DataLoader(train_ds, batch_size=args.batch_size, shuffle=True, collate_fn=data.collate, drop_last=len(train_ds) > args.batch_size)
    val_loader = torch.utils.data.DataLoader(val_ds, batch_size=args.batch_size, shuffle=False, collate_fn=data.collate, drop_last=len(val_ds) > args.batch_size)
    model = model.to(device)
    D.broadcast_parameters(model)
    for m in model.modules():                 # this loop only changes weights through FusedSGD: repack them once per optimizer step,
        if hasattr(m, "repack_policy"):       # not on each of the 64 / batch micro-batch forwards in between
            m.repack_policy = "versioned"
    interval = super_batch_interval(args.batch_size, world)
    steps_per_epoch = optimizer_steps_per_epoch(len(loader), interval)
    opt = FusedSGD(model, lr=args.lr, momentum=args.momentum, nesterov=True, weight_decay=args.weight_decay)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=args.lr, steps_per_epoch=steps_per_epoch, epochs=args.epochs)
    blender = GradientBlender(CoxPH, survival=True, surv_criterion=surv_criterion) if args.blend else None
    # gradients are reduced once per accumulation window: the window's LAST backward is armed, so the all-reduce of a dense block's
    # gradients starts inside that backward as soon as they are final and overlaps the kernels of the blocks still to come
    reducer = D.OverlappedGradientReducer(model) if world > 1 else None
    cat_dim = 1 if args.blend else 0
    best = float("inf")
    for epoch in range(args.epochs):
        model.train()
        losses, c_pred, c_ev, c_du = [], [], [], []
        for i, (x, ev, du) in enumerate(device_batches(loader, device, data.train_tf)):
            out = model(x)
            loss = blender.computeLoss(out, ev, du)[0] if args.blend else surv_criterion(CoxPH, out, ev, du, device)
            boundary = is_step_boundary(i, len(loader), interval)
            if boundary and reducer is not None:
                reducer.arm()
            loss.backward()
            losses.append(loss.detach())
            if boundary:
                if reducer is not None:
                    reducer.finish()
                opt.step()
                sched.step()
                opt.zero_grad()
            c_pred.append(out.detach()); c_ev.append(ev); c_du.append(du)
        cp = torch.cat(c_pred, dim=cat_dim)
        ce, cd = torch.cat(c_ev), torch.cat(c_du)
        tr_c = getCIndices((cp[0] if args.blend else cp).cpu().numpy(), ce.cpu().numpy(), cd.cpu().numpy())
        model.eval()
        y_pred, y_ev, y_du, sel = [], [], [], None
        with torch.no_grad():
            for x, ev, du in device_batches(val_loader, device, data.val_tf):
                p = model(x)
                if args.blend:
                    _, sel = blender.computeLoss(p, ev, du)
                else:
                    sel = surv_criterion(CoxPH, p, ev, du, device)
                y_pred.append(p); y_ev.append(ev); y_du.append(du)
        yp = torch.cat(y_pred, dim=cat_dim)
        ye, yd = torch.cat(y_ev), torch.cat(y_du)
        val_c = getCIndices((yp[0] if args.blend else yp).cpu().numpy(), ye.cpu().numpy(), yd.cpu().numpy())
        sel = float(sel)
        if rank == 0:
            logger.info(f"epoch {epoch + 1}/{args.epochs} train loss/patient {float(torch.stack(losses).sum()) / len(train_ds):.4f} "
                        f"train C {np.nanmean(tr_c):.3f} val selection loss {sel:.4f} val C {np.nanmean(val_c):.3f}")
            if sel < best:
                best = sel
                os.makedirs(args.output_path, exist_ok=True)
                torch.save(model.state_dict(), os.path.join(args.output_path, 'best_surv_model.pth'))
                logger.info('saved new best metric model')
        # every rank evaluates the same epoch-level losses: its own training patients are gathered from all ranks (the
        # validation set is identical on every rank), so one global weight vector results, as on a single GPU
        end_of_epoch(data, rank, blender if args.blend and blender_update_due(epoch, args.blend_update_interval) else None,
                     lambda: (gather_rows(cp, 1, world), gather_rows(ce, 0, world), gather_rows(cd, 0, world), yp, ye, yd))
    if args.blend and rank == 0:
        blender.saveHistory()
    return model


# ---- classification (main.py:125-327) ----------------------------------------------------------------------------------------
def train_classification(model, data, args, device, rank=0, world=1):
    """Binary classification of the event flags: pos-weighted BCE on logits (:147-153), SGD-Nesterov + OneCycleLR stepped every
    batch (:207-215), F1 per class (:217-233,:289-300), best mean validation F1 -> model.pth (:301-306); with --blend the
    GradientBlender's classification branch (:156,:210,:264,:311-314).  With `world` > 1 every rank trains on its own patients:
    identical initial weights, gradients SUM-all-reduced before every optimizer step, checkpoints written by rank 0 only."""
    train_ds, val_ds, bs = data.train, data.val, max(2, args.batch_size)
    loader = torch.utils.data.DataLoader(train_ds, batch_size=bs, shuffle=True, collate_fn=data.collate, drop_last=len(train_ds) > bs)
    val_loader = torch.utils.data.DataLoader(val_ds, batch_size=bs, shuffle=False, collate_fn=data.collate)
    model = model.to(device)
    D.broadcast_parameters(model)
    freqs = torch.tensor(args.class_frequencies, dtype=torch.float32)
    pos_weights = ((torch.ones_like(freqs) - freqs) / freqs).to(device)
    train_loss_function = BCEWithLogitsLoss(pos_weight=pos_weights, reduction='sum')
    loss_function = BCEWithLogitsLoss(pos_weight=pos_weights, reduction='none')
    opt = torch.optim.SGD(model.parameters(), args.lr, momentum=args.momentum, nesterov=True, weight_decay=args.weight_decay)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=args.lr, steps_per_epoch=len(loader), epochs=args.epochs)
    blender = GradientBlender(loss_function, device=device) if args.blend else None
    best_metric, best_epoch = -1.0, -1
    for epoch in range(args.epochs):
        model.train()
        epoch_loss = torch.zeros((), device=device)
        tps = fps = fns = 0
        train_preds, train_gt, val_preds, val_gt = [], [], [], []
        for x, labels, _ in device_batches(loader, device, data.train_tf, targets=1):
            opt.zero_grad()
            outputs = model(x)
            loss = blender.computeLoss(outputs, labels.float()) if args.blend else criterion(train_loss_function, outputs, labels.float(), device)
            loss.backward()
            D.allreduce_gradients(model)
            opt.step()
            sched.step()
            epoch_loss += loss.detach()
            probs = torch.sigmoid(outputs.detach())
            if args.blend:
                train_preds.append(probs); train_gt.append(labels)
                probs = probs[0]
            hit = probs > CLASSIFICATION_THRESHOLD
            tps = tps + (hit & (labels == 1)).sum(0)
            fps = fps + (hit & (labels == 0)).sum(0)
            fns = fns + (~hit & (labels == 1)).sum(0)
        train_f1 = float(np.mean(getF1Score(tps, fps, fns)))
        model.eval()
        test_loss = 0.0
        y_pred, y = [], []
        with torch.no_grad():
            for x, labels, _ in device_batches(val_loader, device, data.val_tf, targets=1):
                p = model(x)
                l = blender.computeLoss(p, labels.float(), no_reduce=True) if args.blend else criterion(loss_function, p, labels.float(), device)
                test_loss += float(l.sum())
                hit = torch.sigmoid(p) > CLASSIFICATION_THRESHOLD
                if args.blend:
                    val_preds.append(hit.float()); val_gt.append(labels)       # thresholded, as upstream :268-272 feeds the blender
                    hit = hit[0]
                y_pred.append(hit); y.append(labels)
        yp, yt = torch.cat(y_pred), torch.cat(y)
        f1s = getF1Score(((yp == 1) & (yt == 1)).sum(0), ((yp == 1) & (yt == 0)).sum(0), ((yp == 0) & (yt == 1)).sum(0))
        mean_f1 = float(np.nanmean(f1s)) if not np.all(np.isnan(f1s)) else 0.0
        if mean_f1 > best_metric:
            best_metric, best_epoch = mean_f1, epoch + 1
            if rank == 0:
                os.makedirs(args.output_path, exist_ok=True)
                torch.save(model.state_dict(), os.path.join(args.output_path, 'model.pth'))
                logger.info('saved new best metric model')
        if rank == 0:
            logger.info(f"epoch {epoch + 1}/{args.epochs} average loss: {float(epoch_loss) / len(train_ds):.4f} train f1 {train_f1:.4f} "
                        f"validation loss {test_loss / len(val_ds):.4f} current f1: {mean_f1:.4f} best f1: {best_metric:.4f} at epoch: {best_epoch}")
        # as in the survival loop: the training patients of all ranks (the validation set is the same everywhere) -> one weight vector
        end_of_epoch(data, rank, blender if args.blend and blender_update_due(epoch, args.blend_update_interval) else None,
                     lambda: (gather_rows(torch.cat(train_preds, dim=1), 1, world), gather_rows(torch.cat(train_gt).float(), 0, world),
                              torch.cat(val_preds, dim=1), torch.cat(val_gt).float()))
    if rank == 0:
        torch.save(model.state_dict(), os.path.join(args.output_path, 'final_model.pth'))
    return model


def inference_survival(model, data, args, device):
    """main.py:750-887: batch-1 loop, Grad-CAM maps (saved as .npy; with `--image_loc` also upstream's per-patient NIfTI folder) of
    fusion and image-only models (main.py:1013-1014: add_gradcam(model, multimodal=...)), C-index."""
    model = model.to(device).eval()
    ds, on_tree = data.evaluation, data.ingest is not None
    cam = add_gradcam(model, multimodal=args.multimodal) if (args.images and not args.no_gradcam) else None
    occ = None
    if args.occlusion:
        occ = add_occlusion(model, multimodal=args.multimodal, window=args.occlusion_window, stride=args.occlusion_stride,
                            batch=args.occlusion_batch)
    preds, evs, dus = [], [], []
    os.makedirs(os.path.join(args.output_path, "attention_maps"), exist_ok=True)
    for i, (x, ev, du) in enumerate(device_batches((data.collate([ds[j]]) for j in range(len(ds))), device, data.val_tf, targets=0)):
        folder = patient_folder(args.output_path, ds.uids[i]) if on_tree else None
        with torch.no_grad():
            if cam is not None:
                p, maps = cam(x)
                # fusion: the list of per-class maps, the first saved; image-only: (1, 1, D, H, W), the sample's map saved
                att = maps[0] if args.multimodal else maps[0, 0]
                np.save(os.path.join(args.output_path, "attention_maps", f"patient{i}_att_map.npy"), att.cpu().numpy())
                if on_tree:
                    export_patient_nifti(folder, (x["image"] if args.multimodal else x)[0], att, p)
                if args.scan_space:
                    # the maps live in the space of the ingest's S^3 planes: `--transforms` puts only the validation transforms
                    # between the two, and those are spatially the identity at S^3 (intensity stages and a Resize to the size the
                    # planes already have: both take `--image_size`), so the map needs no further correction.  Fusion: one map per class; image-only: the
                    # sample's one map, class 0
                    stack = torch.stack(list(maps)) if args.multimodal else maps[0]
                    export_scan_space_maps(folder, stack.contiguous(), data.ingest.last_volumes[0])
            elif occ is None:
                p = model(x)
            if occ is not None:
                # the occluded inputs are built from what the model sees: the batch after the validation transforms
                outs, occ_maps = occ(x)
                if cam is None:
                    p = outs
                np.save(os.path.join(args.output_path, "attention_maps", f"patient{i}_occ_map.npy"), occ_maps.cpu().numpy())
                if on_tree:
                    export_occlusion_nifti(folder, occ_maps)
                if args.scan_space:
                    export_scan_space_maps(folder, occ_maps, data.ingest.last_volumes[0], prefix="occ_map")
        preds.append(p.cpu()); evs.append(ev); dus.append(du)
    p, e, d = torch.cat(preds).numpy(), torch.cat(evs).numpy(), torch.cat(dus).numpy()
    report_empty_masks(data.ingest)
    if args.bootstrap:
        means, stds, used = bootstrap_c_indices(p, e, d)
        logger.info('Mean c indices: {}'.format(means))
        logger.info('Std. devs: {} ({} of {} resamples had admissible pairs)'.format(stds, used, NUM_BOOTSTRAP_ITERATIONS))
    else:
        logger.info('All C-indexes: {}'.format(getCIndices(p, e, d)))
    return p


class SyntheticImagePatients(SyntheticPatients):
    """Synthetic image patients addressed by uid (0 .. n-1) with three event flags each: the shape of the image classification
    dataset upstream's find_lr trains its 3-class DenseNet121 on (utils/find_lr.py:25,96-100)."""

    def __init__(self, n, in_channels, size, seed, classes=3):
        super().__init__(n, in_channels, size, 0, False, True, seed)
        g = torch.Generator().manual_seed(seed + 1)
        self.events = (torch.rand((n, classes), generator=g) < 0.6).long()
        self.uids = list(range(n))


def run_lr_finder(a):
    """`--lr_finder` (upstream main.py:1009-1010 -> utils/find_lr.py): the range test of a fresh 3-class MONAI-schema DenseNet121 on
    synthetic patients, then lr_finder.csv (lr,loss per recorded iteration), lr_finder.png and the suggested lr."""
    from mmnn_sts_amd.utils.find_lr import find_lr
    if not torch.cuda.is_available():
        raise SystemExit(NO_DEVICE)
    torch.cuda.set_device(0)
    ds = SyntheticImagePatients(max(2, a.synthetic_patients), a.in_channels, a.synthetic_size, TRAIN_SEED)
    os.makedirs(a.output_path, exist_ok=True)
    finder, suggestion = find_lr(a, ds)                  # (reads a.seed, a.in_channels, a.batch_size, a.output_path)
    with open(os.path.join(a.output_path, "lr_finder.csv"), "w") as f:
        f.write("lr,loss\n")
        for lr, loss in zip(finder.history["lr"], finder.history["loss"]):
            f.write(f"{lr!r},{loss!r}\n")
    if suggestion is not None:
        logger.info("Suggested LR: %.2E", suggestion)
    else:
        logger.info("Suggested LR: none (too few points)")
    return finder


def build_arg_parser():
    ap = argparse.ArgumentParser()
    for flag, h in (("preop", "clinical features available pre-operation"), ("postop", "pre + post operation clinical features"),
                    ("radiomics", "radiomic features: the csv of --rad_loc, or extracted on the device from --image_loc"), ("images", "image data"),
                    ("classification", "binary classification"), ("survival", "time-to-event model"), ("segmentation", "unsupported"),
                    ("lr_finder", "learning-rate range test (with --images --classification): lr_finder.csv / .png, suggested lr"), ("no_gradcam", "disable Grad-CAM for inference"), ("inference", "inference"),
                    ("split", "create a new dataset split"), ("blend", "gradient blending"), ("bootstrap", "bootstrap evaluation (with --inference --survival)")):
        ap.add_argument(f"--{flag}", action="store_true", help=h)
    for twin in ("use_images", "use_preop", "use_postop", "classification_task", "inference_task", "survival_task", "use_blend"):
        ap.add_argument(f"--{twin}", type=str, default="false")
    ap.add_argument("--weights", type=str, default=None)
    ap.add_argument("--output_path", type=str, default=".")
    for loc in ("data_loc", "image_loc", "key_loc", "rad_loc"):
        ap.add_argument(f"--{loc}", type=str, default=None)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--train_uid_location", type=str, default="./stratified_train_uids.txt")
    ap.add_argument("--val_uid_location", type=str, default="./stratified_val_uids.txt")
    ap.add_argument("--config", type=str, default=None)
    ap.add_argument("--blend_update_interval", type=int, default=5)
    ap.add_argument("--transforms", action="store_true",
                    help="run upstream's train_transforms / val_transforms on every image batch on the device (resizes to 64^3, or to "
                         "the extent of --image_size)")
    ap.add_argument("--image_size", type=int, default=None,
                    help="extent S per axis, 1..128, of the volumes the model sees (default 64; overrides the config's `Data: size`): "
                         "with --image_loc the scans are ingested at S^3, without it the synthetic patients are S^3; --transforms resizes "
                         "to S^3 and the attention / occlusion maps and their exports are S^3")
    ap.add_argument("--cache_volumes", action="store_true",
                    help="with --image_loc: ingest each patient once and keep its S^3 planes on the device; later epochs assemble their "
                         "batches there and open no file (also `Data: cache: true`).  Patients beyond --cache_gb are read every epoch")
    ap.add_argument("--cache_gb", type=float, default=None,
                    help="budget of --cache_volumes in GB (default 16; overrides the config's `Data: cache_gb`): 2 MB per patient at 2 x 64^3")
    ap.add_argument("--scan_space", action="store_true",
                    help="with --inference --image_loc and Grad-CAM on: also write every class's attention map on each scan's own voxel "
                         "grid, with the scan's affine (att_map_class{k}_on_{t1,t2,scan}.nii.gz)")
    ap.add_argument("--occlusion", action="store_true",
                    help="with --inference --images: occlusion sensitivity maps per patient (attention_maps/patient{i}_occ_map.npy, "
                         "(K, D, H, W) signed deltas; with --image_loc occ_map_class{k}.nii.gz, with --scan_space also on the scans' grids)")
    from mmnn_sts_amd.radiomics import add_extraction_arguments
    add_extraction_arguments(ap, "with --radiomics and no --rad_loc: ")
    ap.add_argument("--mask_margin_mm", type=float, default=None,
                    help="with --image_loc: dilate every mask by this many mm on the device ahead of the scan ingest, so the volumes show the "
                         "tumour and the rim around it; overrides the config's `Data: mask_margin_mm` (the radiomics ROI is not changed)")
    ap.add_argument("--occlusion_window", type=int, default=16, help="edge of the occluded box in voxels")
    ap.add_argument("--occlusion_stride", type=int, default=8, help="step of the box, 1..window")
    ap.add_argument("--occlusion_batch", type=int, default=8, help="occluded samples per forward")
    # synthetic-data knobs (no counterpart upstream)
    ap.add_argument("--synthetic_patients", type=int, default=16)
    ap.add_argument("--synthetic_size", type=int, default=64)
    return ap


@contextlib.contextmanager
def configuration_errors_exit():
    """A setting the config layer refuses ends the command line with its message."""
    try:
        yield
    except ConfigurationError as e:
        raise SystemExit(str(e))


def resolve_settings(a, parser):
    """Every check of the command line against itself and the config, in the one order that decides which message a user sees, and every
    setting derived from the two: `a` comes back as the record of the run, which nothing later assigns to.  Beyond the flags it holds
    `use_nifti` (the run reads patient directories), `multimodal`, `seed`, `in_channels`, `batch_size`, `momentum`, `weight_decay` and
    `class_frequencies`; `image_size`, `synthetic_size`, `mask_margin_mm`, `cache_volumes`, `cache_gb`, `blend` and `no_gradcam` hold
    what the run uses.  Reads the config (`parser.parseConfig`) and lays the location flags over its `Data:` section."""
    a.images = a.images or str_to_bool(a.use_images)
    a.classification = a.classification or str_to_bool(a.classification_task)
    a.inference = a.inference or str_to_bool(a.inference_task)
    a.survival = a.survival or str_to_bool(a.survival_task)
    a.preop = a.preop or str_to_bool(a.use_preop)
    a.postop = a.postop or str_to_bool(a.use_postop)
    a.blend = a.blend or str_to_bool(a.use_blend)
    assert not all([a.classification, a.survival, a.segmentation]), 'Can only specify one of --classification , --survival , or --segmentation'
    assert any([a.classification, a.survival, a.segmentation]), 'Must specify one of --classification , --survival , or --segmentation'
    if a.segmentation:
        raise SystemExit("--segmentation is outside the MI355X fusion path (SURVEY 2)")
    if a.lr_finder and not (a.images and a.classification and not (a.preop or a.postop)):
        raise SystemExit("--lr_finder runs upstream's find_lr on an image classification dataset: it needs --images --classification "
                         "and no clinical flags (--preop / --postop)")
    if a.lr_finder and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--lr_finder is single-process (as upstream's find_lr); run it without torch.distributed.run")
    if a.bootstrap and not (a.inference and a.survival):
        raise SystemExit("--bootstrap resamples the evaluation of `--inference --survival` (main.py:767-887); it has no meaning for training runs")
    if a.occlusion:
        missing = [f for f, on in (("--inference", a.inference), ("--images", a.images)) if not on]
        if missing:
            raise SystemExit("--occlusion writes occlusion sensitivity maps of the image input at inference: it needs " + " and ".join(missing))
        if a.bootstrap:
            raise SystemExit("--occlusion excludes --bootstrap (bootstrapping writes no maps, main.py:774-777)")
        if not (1 <= a.occlusion_stride <= a.occlusion_window) or a.occlusion_batch < 1:
            raise SystemExit(f"--occlusion needs 1 <= --occlusion_stride ({a.occlusion_stride}) <= --occlusion_window ({a.occlusion_window}) "
                             f"and --occlusion_batch ({a.occlusion_batch}) >= 1")
    if a.transforms and not a.images:
        raise SystemExit("--transforms acts on image volumes: it needs --images")

    cfg = parser.parseConfig()
    data_cfg = parser.applyDataFlags(a)
    if a.radiomics:             # the csv of --rad_loc / `Data: rad_loc`, or an image tree to extract it from; the clinical csv holds the targets
        if not data_cfg.get("rad_loc") and not data_cfg.get("image_loc"):
            raise SystemExit("--radiomics needs --rad_loc (a csv of radiomic features with the column MRN) or --image_loc (patient directories "
                             "to extract the features from)")
        if not data_cfg.get("rad_loc") and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--radiomics without --rad_loc extracts the features in a single process: run the extraction once "
                             "(python -m mmnn_sts_amd.radiomics) and pass its csv as --rad_loc")
        missing = [k for k in (("data_loc",) if data_cfg.get("rad_loc") else ("data_loc", "key_loc")) if not data_cfg.get(k)]
        if missing:
            raise SystemExit("--radiomics needs " + " and ".join(f"--{k}" for k in missing) + " (the clinical csv with uid, event{i}, duration{i}"
                             + ("" if data_cfg.get("rad_loc") else "; the patient key csv with the columns 'Anon MRN', 'MRN'") + ")")
        if a.images and not data_cfg.get("image_loc"):
            raise SystemExit("--radiomics with --images pairs each patient's features with their scans: it needs --image_loc")
        if a.lr_finder:
            raise SystemExit("--lr_finder runs on synthetic image patients: run it without --radiomics")
    # (--radiomics without --images reads --image_loc only to extract its features from)
    a.use_nifti = bool(data_cfg.get("image_loc")) and (bool(a.image_loc) or a.images) and (a.images or not a.radiomics)
    # --cache_volumes / `Data: cache` and its budget --cache_gb / `Data: cache_gb` (16 when not named)
    a.cache_volumes = a.cache_volumes or bool(data_cfg.get("cache"))
    gb = a.cache_gb if a.cache_gb is not None else data_cfg.get("cache_gb")
    if gb is not None and not a.cache_volumes:
        raise SystemExit("--cache_gb is the budget of the volume cache: it needs --cache_volumes")
    if a.cache_volumes:
        if not a.use_nifti:
            raise SystemExit("--cache_volumes keeps the ingested scans of patient directories on the device: it needs --image_loc")
        if a.inference:
            raise SystemExit("--cache_volumes saves the re-reading of patients in later epochs: --inference reads each patient once, run it without")
        if a.lr_finder:
            raise SystemExit("--cache_volumes caches ingested patient scans: --lr_finder runs on synthetic patients, run it without")
        gb = DEFAULT_CACHE_GB if gb is None else gb
        if isinstance(gb, bool) or not isinstance(gb, (int, float)) or not 0 < gb < float("inf"):
            raise SystemExit(f"--cache_gb {gb!r} is not a positive number of GB")
        a.cache_gb = float(gb)
    with configuration_errors_exit():
        a.mask_margin_mm = parser.maskMargin(a.mask_margin_mm)
        parser.radiomicsShell(a.shell_mm)               # (refused here; `Parser.radiomicsExtraction` resolves the widths for the extraction)
    if a.mask_margin_mm is not None and not a.use_nifti:
        raise SystemExit("--mask_margin_mm / `Data: mask_margin_mm` widens the masks of patient directories: it needs --image_loc (synthetic "
                         "patients have no mask)")
    if a.shell_mm is not None and not (a.radiomics and not data_cfg.get("rad_loc")):
        raise SystemExit("--shell_mm adds columns to the table extracted on the device: it needs --radiomics and no "
                         "--rad_loc")
    a.in_channels = int(cfg["ImageModel"]["in_channels"])
    if a.use_nifti:
        if not a.images:
            raise SystemExit("--image_loc points at NIfTI patient directories: it needs --images")
        missing = [k for k in ("key_loc", "data_loc") if not data_cfg.get(k)]
        if missing:
            raise SystemExit("--image_loc needs " + " and ".join(f"--{k}" for k in missing) + " (the patient key csv with the columns "
                             "'Anon MRN', 'MRN'; the clinical csv with uid, predictors, event{i}, duration{i})")
        if a.lr_finder:
            raise SystemExit("--lr_finder runs on synthetic patients: run it without --image_loc")
        n_mod = 2 if cfg["ImageModel"]["modality"].lower().startswith("t1t2") else 1
        if a.in_channels != n_mod:
            raise SystemExit(f"ImageModel modality {cfg['ImageModel']['modality']} yields {n_mod} channel(s) per patient, in_channels is {cfg['ImageModel']['in_channels']}")
    if a.scan_space and not (a.inference and a.use_nifti and a.images and not a.no_gradcam and not a.bootstrap):
        raise SystemExit("--scan_space lays the Grad-CAM attention maps over the patients' scans: it needs --inference, --image_loc (NIfTI "
                         "patient directories) and Grad-CAM on (--images, neither --no_gradcam nor --bootstrap)")
    # the extent S of the image volumes: named by --image_size / `Data: size`, else 64 for the ingest and the Resize (and
    # --synthetic_size for synthetic patients, as before)
    sized = a.image_size is not None or (data_cfg.get("size") is not None)
    if sized and not a.images:
        raise SystemExit("--image_size / `Data: size` is the extent of the image volumes: it needs --images")
    if a.images:
        with configuration_errors_exit():
            a.image_size = parser.imageSize(a.image_size)
        if sized and not a.use_nifti:
            a.synthetic_size = a.image_size
    hp = cfg.get("Hyperparameters", {})
    a.multimodal = a.images and (a.preop or a.postop or a.radiomics)
    a.blend = a.blend and a.multimodal
    a.no_gradcam = a.no_gradcam or a.bootstrap      # main.py:774-777: no attention maps, no prediction dump while bootstrapping
    a.batch_size = int(hp.get("train_batch_size", 2)) if a.config else 2
    a.momentum, a.weight_decay = float(hp.get("momentum", 0.9)), float(hp.get("weight_decay", 1e-4))
    a.class_frequencies = list(hp.get("class_frequencies", [0.4] * NUM_CLASSES))     # CLASS_FREQUENCIES is undefined upstream (Q1)
    a.seed = int(hp.get("seed", 42))
    return a


def main(argv=None):
    a = build_arg_parser().parse_args(argv)
    parser = Parser(a.config)
    resolve_settings(a, parser)
    torch.manual_seed(a.seed)
    if a.lr_finder:
        return run_lr_finder(a)
    if a.radiomics:
        extract_radiomics_if_needed(parser, a)
    model = parser.getModel(a)
    if a.multimodal:
        model.blend = a.blend
    rank, world, local = D.init_from_env(os.environ.get("MMNN_DIST_BACKEND", "nccl"))    # "nccl" = RCCL; gloo only for rehearsals on one card
    if not torch.cuda.is_available():
        raise SystemExit(NO_DEVICE)
    local = local % max(1, torch.cuda.device_count())            # (gloo rehearsals: several ranks share a card)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if a.weights:
        model = loadWeights(model, a.weights, "cpu")
    data = build_data_source(a, parser, rank, world, device)
    if a.inference:
        inference_survival(model, data, a, device)
    elif a.survival:
        train_survival(model, data, a, device, rank, world)
    else:
        train_classification(model, data, a, device, rank, world)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
