"""The clinical csv of this project (main.py: `write_synthetic_csv`): one row per patient -- `uid`, the predictor columns, then per target
`event{i}` and `duration{i}` -- addressed by uid, as upstream's data/ClinicalDatasets.py:6-89 addresses its own csv.  (Upstream's csv --
dates, one-hot columns, hospital headers -- cannot be reproduced and is not read.)"""
import numpy as np
import torch

from ..exceptions.exceptions import ConfigurationError
from .constants import NUM_CLASSES


class LabelTable:
    """uid -> (events, durations) and the predictor columns of one clinical csv."""

    def __init__(self, path):
        self.path = str(path)
        with open(self.path) as f:
            self.header = f.readline().strip().split(",")
        self.table = np.loadtxt(self.path, delimiter=",", skiprows=1, ndmin=2)
        self.col = {name: i for i, name in enumerate(self.header)}
        need = ["uid"] + [f"event{i}" for i in range(NUM_CLASSES)] + [f"duration{i}" for i in range(NUM_CLASSES)]
        missing = [c for c in need if c not in self.col]
        if missing:
            raise ConfigurationError(f"clinical csv {self.path} lacks the columns {missing}")
        self.row = {int(u): r for r, u in enumerate(self.table[:, self.col["uid"]])}

    @property
    def uids(self):
        return list(self.row)

    def _row(self, uid):
        if int(uid) not in self.row:
            raise ConfigurationError(f"patient uid {uid} has no row in the clinical csv {self.path}")
        return self.table[self.row[int(uid)]]

    def events(self, uid):
        return torch.from_numpy(self._row(uid)[[self.col[f"event{i}"] for i in range(NUM_CLASSES)]]).long()

    def durations(self, uid):
        return torch.from_numpy(self._row(uid)[[self.col[f"duration{i}"] for i in range(NUM_CLASSES)]]).long()

    def predictors(self, uid, names):
        missing = [p for p in names if p not in self.col]
        if missing:
            raise ConfigurationError(f"clinical csv {self.path} lacks predictor columns {missing[:4]}...")
        return torch.from_numpy(self._row(uid)[[self.col[p] for p in names]]).float()


class ClinicalDataset(torch.utils.data.Dataset):
    """(features, events, durations) with `survival`, else (features, labels = the event flags)."""

    def __init__(self, filename, predictors, classification=False, survival=False):
        self.labels = LabelTable(filename)
        self.predictors = list(predictors)
        self.survival = survival and not classification
        self.multimodal_identifier = 'clinical'
        self._uids = self.labels.uids

    @property
    def uids(self):
        return self._uids

    def __len__(self):
        return len(self._uids)

    def getDataByUID(self, uid):
        x = self.labels.predictors(uid, self.predictors)
        if self.survival:
            return x, self.labels.events(uid), self.labels.durations(uid)
        return x, self.labels.events(uid)

    def __getitem__(self, index):
        return self.getDataByUID(self._uids[index])
