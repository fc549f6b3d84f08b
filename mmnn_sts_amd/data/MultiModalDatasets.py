"""data/MultiModalDatasets.py:8-86: one item per uid common to all member datasets, {multimodal_identifier: data} plus the targets, which
must agree between the members."""
import torch

from ..exceptions.exceptions import ConfigurationError


class MultiModalDataset(torch.utils.data.Dataset):
    n_targets = 1

    def __init__(self, datasets, transforms=None):
        if transforms is not None:
            raise ConfigurationError("per-item transforms cannot run on raw voxels: pass --transforms (they act on the collated device batch)")
        self.datasets = list(datasets)
        common = set.intersection(*(set(d.uids) for d in self.datasets))
        self.mrns = sorted(common)

    def __len__(self):
        return len(self.mrns)

    @property
    def uids(self):
        return self.mrns

    @property
    def clinical_dataset(self):
        for dataset in self.datasets:
            if dataset.multimodal_identifier == 'clinical':
                return dataset
        raise ValueError("none of the member datasets is the clinical one (multimodal_identifier 'clinical')")

    def getDataByUID(self, uid):
        data, targets = {}, None
        for dataset in self.datasets:
            item = dataset.getDataByUID(uid)
            data[dataset.multimodal_identifier] = item[0]
            new = tuple(item[1:1 + self.n_targets])
            if targets is not None:
                assert all(torch.all(a == b) for a, b in zip(new, targets)), \
                    f'the member datasets disagree on the targets of patient {uid}'
            else:
                targets = new
        return (data, *targets)

    def __getitem__(self, index):
        return self.getDataByUID(self.mrns[index])


class MultiModalSurvivalDataset(MultiModalDataset):
    """({'image', 'clinical'}, events, durations)."""
    n_targets = 2
