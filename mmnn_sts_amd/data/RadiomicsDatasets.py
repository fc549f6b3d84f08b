"""data/RadiomicsDatasets.py of upstream, over a csv of radiomic features: one row per patient, the column `MRN` (the uid) and the feature
columns -- what `mmnn_sts_amd.radiomics.extract_tree` writes, or a PyRadiomics csv that has been given an `MRN` column.  Upstream's
class names and constructor arguments; the targets come from this project's clinical csv (`LabelTable`).

Columns named `diagnostics_*` (PyRadiomics' provenance columns) and any named in `RadiomicsModel: RADIOMICS_EXCLUDE_COLUMNS` /
`RADIOMICS_LABEL_COLUMNS` are dropped; what remains must be finite numbers, or the constructor names the patient and the column.
`fit_scaler` / `set_scaler` / `save_scaler` / `load_scaler`: z-scoring with the mean and standard deviation of the training uids (a
standard deviation of 0 is taken as 1), kept in `radiomics_scaler.csv`.  `JoinedTableDataset`: clinical and radiomic columns of the
patients common to both, clinical first, as one predictor table."""
import csv
import math

import numpy as np
import torch

from ..exceptions.exceptions import ConfigurationError
from .ClinicalDatasets import LabelTable

UID_COLUMN = "MRN"
SCALER_FILE = "radiomics_scaler.csv"


def feature_columns(header, exclude=()):
    drop = {UID_COLUMN, *exclude}
    return [c for c in header if c not in drop and not c.startswith("diagnostics_")]


class RadiomicsDataset(torch.utils.data.Dataset):
    """(features, labels = the event flags)."""
    survival = False

    def __init__(self, radiomics_path, clinical_data, exclude_columns=(), label_columns=()):
        self.path = str(radiomics_path)
        with open(self.path, newline="") as f:
            rows = [r for r in csv.reader(f) if r]
        if not rows or UID_COLUMN not in rows[0]:
            raise ConfigurationError(f"radiomics csv {self.path} has no column {UID_COLUMN!r}")
        header = [c.strip() for c in rows[0]]
        self.columns = feature_columns(header, tuple(exclude_columns) + tuple(label_columns))
        if not self.columns:
            raise ConfigurationError(f"radiomics csv {self.path} has no feature column")
        at = {c: i for i, c in enumerate(header)}
        self.row, table = {}, []
        for r in rows[1:]:
            try:
                uid = int(float(r[at[UID_COLUMN]]))
            except (ValueError, IndexError):
                raise ConfigurationError(f"radiomics csv {self.path}: {UID_COLUMN} {r[at[UID_COLUMN]] if len(r) > at[UID_COLUMN] else ''!r} is not a patient uid")
            values = []
            for c in self.columns:
                try:
                    v = float(r[at[c]])
                except (ValueError, IndexError):
                    v = float("nan")
                if not math.isfinite(v):
                    cell = r[at[c]] if len(r) > at[c] else ""
                    raise ConfigurationError(f"radiomics csv {self.path}: patient {uid}, column {c}: {cell!r} is not a finite number")
                values.append(v)
            if uid in self.row:
                raise ConfigurationError(f"radiomics csv {self.path}: patient {uid} has two rows")
            self.row[uid] = len(table)
            table.append(values)
        self.table = np.asarray(table, dtype=np.float64).reshape(len(table), len(self.columns))
        self.labels = LabelTable(clinical_data)
        missing = [u for u in self.row if u not in self.labels.row]
        if missing:
            raise ConfigurationError(f"patients {missing[:8]} of {self.path} have no row in the clinical csv {clinical_data}")
        self.multimodal_identifier = "clinical"          # the tabular input of the models, whichever table it comes from
        self.mean = np.zeros(len(self.columns))
        self.std = np.ones(len(self.columns))

    @property
    def uids(self):
        return list(self.row)

    @property
    def predictors(self):
        return list(self.columns)

    def __len__(self):
        return len(self.row)

    # ---- the scaler ------------------------------------------------------------------------------------------------------------------
    def fit_scaler(self, train_uids):
        rows = [self.row[int(u)] for u in train_uids if int(u) in self.row]
        if not rows:
            raise ConfigurationError(f"none of the training uids has a row in {self.path}")
        mean, std = self.table[rows].mean(axis=0), self.table[rows].std(axis=0)
        self.set_scaler(mean, np.where(std == 0.0, 1.0, std))
        return self.mean, self.std

    def set_scaler(self, mean, std):
        self.mean, self.std = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(std, dtype=np.float64).reshape(-1)
        if self.mean.shape != (len(self.columns),) or self.std.shape != (len(self.columns),):
            raise ConfigurationError(f"a scaler of {self.mean.size} columns does not fit the {len(self.columns)} feature columns of {self.path}")

    def save_scaler(self, path):
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["column", "mean", "std"])
            for c, m, s in zip(self.columns, self.mean, self.std):
                w.writerow([c, repr(float(m)), repr(float(s))])

    def load_scaler(self, path):
        with open(path, newline="") as f:
            rows = [r for r in csv.reader(f) if r][1:]
        if [r[0] for r in rows] != self.columns:
            raise ConfigurationError(f"the scaler {path} was fitted on other columns than those of {self.path}")
        self.set_scaler([float(r[1]) for r in rows], [float(r[2]) for r in rows])

    # ---- items -----------------------------------------------------------------------------------------------------------------------
    def features(self, uid):
        if int(uid) not in self.row:
            raise ConfigurationError(f"patient uid {uid} has no row in the radiomics csv {self.path}")
        return torch.from_numpy((self.table[self.row[int(uid)]] - self.mean) / self.std).float()

    def getDataByUID(self, uid):
        if self.survival:
            return self.features(uid), self.labels.events(uid), self.labels.durations(uid)
        return self.features(uid), self.labels.events(uid)

    def __getitem__(self, index):
        return self.getDataByUID(self.uids[index])


class RadiomicsSurvivalDataset(RadiomicsDataset):
    """(features, events, durations)."""
    survival = True


class RadiomicsClassificationDataset(RadiomicsDataset):
    """(features, labels)."""


class JoinedTableDataset(torch.utils.data.Dataset):
    """Two predictor tables joined on uid, the first one's columns first (clinical, then radiomic)."""

    def __init__(self, tables):
        self.tables = list(tables)
        self.multimodal_identifier = "clinical"
        self._uids = sorted(set.intersection(*(set(t.uids) for t in self.tables)))
        self.predictors = [p for t in self.tables for p in t.predictors]

    @property
    def uids(self):
        return self._uids

    def __len__(self):
        return len(self._uids)

    def getDataByUID(self, uid):
        items = [t.getDataByUID(uid) for t in self.tables]
        for other in items[1:]:
            assert all(torch.all(a == b) for a, b in zip(items[0][1:], other[1:])), f"the tables disagree on the targets of patient {uid}"
        return (torch.cat([it[0] for it in items]), *items[0][1:])

    def __getitem__(self, index):
        return self.getDataByUID(self._uids[index])


class TableByUIDs(torch.utils.data.Dataset):
    """The sub-dataset of a table (or of a multimodal dataset) that reaches the given uids only; classification items get a third
    element (None) so that every loop unpacks (x, targets, durations)."""

    def __init__(self, dataset, uids):
        self.dataset, self.set_uids = dataset, [int(u) for u in uids]
        known = set(dataset.uids)
        missing = [u for u in self.set_uids if u not in known]
        if missing:
            raise ConfigurationError(f"uids {missing[:8]} are not in the dataset")

    @property
    def uids(self):
        return self.set_uids

    def __len__(self):
        return len(self.set_uids)

    def __getitem__(self, index):
        item = self.dataset.getDataByUID(self.set_uids[index])
        return item if len(item) == 3 else (*item, item[1])
