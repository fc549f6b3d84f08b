"""Upstream's local-disk image datasets (data/ImageDatasets.py:26-56, 196-292, 310-377, 422-470, 520-640) with their class names and
constructor arguments.  The directory contract is upstream's: one directory per patient under `patient_directory`, in one of two layouts,
detected per tree (`Data: format: auto | nifti | dicom` forces one; a tree that mixes them is refused):

    NIfTI   the file whose name starts with `scan` is the image and the other one the mask; the anonymised id is the first two
            `-`-separated fields of the directory name (:426)
    DICOM   the sub-directories `image` and `mask` each hold one series, `<series>/*.dcm` or the files themselves (:26-56); the
            anonymised id is the directory name when the key has it (data/utils.py:8-14), else as for NIfTI.  Uncompressed
            single-frame series only (`mmnn_sts_amd.data.dicom`); the mask is a DICOM image series too, always resampled into the
            scan's grid and binarised at 128 by default -- or one RT Structure Set file (`mmnn_sts_amd.data.rtstruct`): `mask/` (or
            its single sub-directory) then holds no image file and exactly one RTSTRUCT file, whose ROI `mask_roi` (`Data: mask_roi`;
            None: its only ROI) is rasterised onto the scan's own grid on the device and takes neither resample nor threshold --
            or one DICOM Segmentation file (`mmnn_sts_amd.data.seg`, BINARY only); one scan of `mask/` tells the three apart by
            SOP class (`mask_source`).  The frames of the
            segment `mask_roi` names by its SegmentLabel are unpacked on the device, straight onto the scan's grid when they lie
            on its slice planes, else onto the segmentation's own grid and then resampled like a mask series.  A NIfTI mask beside a
            DICOM scan, enhanced multi-frame scans, FRACTIONAL / LABELMAP SEG and compressed syntaxes are outside the path

`patient_key` is a csv with the columns `Anon MRN` and `MRN` that maps the anonymised id to the uid.  Labels come from this project's
clinical csv (`ClinicalDatasets.LabelTable`), joined on `uid`.  `ImageClassificationDataset` / `ImageSurvivalDataset` are upstream's
names of the DICOM-layout classes; unlike upstream's, the survival one masks like its classification twin.

`__getitem__` yields a `RawPatient` -- the files' voxels in their on-disk type, unmasked and uncropped -- in place of upstream's float
volume: masking, empty-slice removal, the area resize (to 64^3, or to the S^3 of `IngestCollate(size=S)`) and the T1 / T2 stacking happen
on the device in the collate function (`mmnn_sts_amd.data.ingest.IngestCollate`), and upstream's train / validation transforms act on the collated batch (`--transforms`).
`transforms`, `slices` are accepted for signature parity; a per-item transform cannot run on raw voxels and is refused.

A mask whose extents differ from its scan's (drawn on another series, resliced, cropped to the tumour's bounding box) is accepted when
both files carry a qform / sform: the collate function resamples it into the scan's grid on the device, as upstream's DICOM datasets do
with `sitk.Resample(mask, image)` (:145-152).  `mask_resample` is the `Data:` key of that name: 'auto' (the default), 'geometry', 'never'.
"""
import csv
import logging
import os

import torch

from ..exceptions.exceptions import ConfigurationError
from . import dicom, nifti, rtstruct, seg
from .ClinicalDatasets import LabelTable
from .ingest import MASK_RESAMPLE_MODES, RawPatient

logger = logging.getLogger(__name__)
RADIOMICS_UID = 'MRN'
ANON_ID = 'Anon MRN'
FORMATS = ('auto', 'nifti', 'dicom')


def anon_id_of(directory_name):
    return '-'.join(directory_name.split('-')[:2])


def _read_key(path):
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    if not rows or ANON_ID not in rows[0] or RADIOMICS_UID not in rows[0]:
        raise ConfigurationError(f"patient key {path} needs the columns '{ANON_ID}' and '{RADIOMICS_UID}'")
    return {r[ANON_ID].strip(): int(float(r[RADIOMICS_UID])) for r in rows}


def layout_of(patient_path):
    """'dicom' (the sub-directories `image` and `mask`), 'nifti' (a file named scan*) or None for one patient directory."""
    entries = [e for e in os.listdir(patient_path) if not e.startswith('.')]
    is_dicom = all(os.path.isdir(os.path.join(patient_path, d)) for d in ('image', 'mask'))
    is_nifti = any(e.startswith('scan') and os.path.isfile(os.path.join(patient_path, e)) for e in entries)
    if is_dicom and is_nifti:
        raise ConfigurationError(f"{patient_path} holds both the DICOM layout (image/, mask/) and a NIfTI scan*: one format per tree")
    if os.path.isdir(os.path.join(patient_path, 'image')) and not is_dicom:
        raise ConfigurationError(f"{patient_path}: image/ without a mask/ directory beside it (a NIfTI mask beside a DICOM scan is outside "
                                 "the path; an RTSTRUCT or DICOM SEG file belongs into mask/)")
    return 'dicom' if is_dicom else ('nifti' if is_nifti else None)


def mask_source(mask_directory):
    """What `mask_directory` (or its single sub-directory) holds, from one scan of it: ('series', the directory), ('rtstruct', the RT
    Structure Set file) or ('seg', the DICOM Segmentation file).  Dot files and files without the magic are skipped; the others are
    told apart by SOPClassUID alone (`seg.sop_class_of`), so a SEG file never reaches `dicom.read_file`, which refuses multi-frame
    objects.  Refused: several RTSTRUCT or several SEG files, a SEG file beside an RTSTRUCT file, either beside image files.  A
    directory with neither is a series, whatever else is wrong with it: `dicom.read_series` reports that."""
    try:
        d = dicom.series_directory(mask_directory)
    except ConfigurationError:
        return 'series', str(mask_directory)
    found = {seg.SEGMENTATION_STORAGE: [], rtstruct.RT_STRUCTURE_SET_STORAGE: []}
    others = []
    for name in sorted(os.listdir(d)):
        p = os.path.join(d, name)
        if name.startswith('.') or not os.path.isfile(p):
            continue
        try:
            found.get(seg.sop_class_of(p), others).append(p)
        except dicom.NotDicomError:
            continue
    segs, sets = (found[k] for k in (seg.SEGMENTATION_STORAGE, rtstruct.RT_STRUCTURE_SET_STORAGE))
    if not segs and not sets:
        return 'series', str(mask_directory)
    if len(segs) > 1:
        raise ConfigurationError(f"{d}: {len(segs)} DICOM SEG files ({', '.join(os.path.basename(p) for p in segs[:4])}): one segmentation per mask/ is expected")
    if segs and sets:
        raise ConfigurationError(f"{d}: a DICOM SEG file ({os.path.basename(segs[0])}) beside an RTSTRUCT file ({os.path.basename(sets[0])}): "
                                 "mask/ holds one image series, one structure set or one segmentation")
    if len(sets) > 1:
        raise ConfigurationError(f"{d}: {len(sets)} RTSTRUCT files ({', '.join(os.path.basename(p) for p in sets[:4])}): one structure set per mask/ is expected")
    images = sum(1 for p in others if dicom.read_file(p, header_only=True).has_image)
    if images and segs:
        raise ConfigurationError(f"{d}: a DICOM SEG file ({os.path.basename(segs[0])}) beside {images} DICOM image file(s): mask/ holds one "
                                 "image series, one structure set or one segmentation")
    if images:
        raise ConfigurationError(f"{d}: an RTSTRUCT file ({os.path.basename(sets[0])}) beside {images} DICOM image file(s): mask/ holds either "
                                 "one image series or one structure set")
    return ('seg', segs[0]) if segs else ('rtstruct', sets[0])


def rtstruct_in(mask_directory):
    """The path of the RT Structure Set file when `mask_source` finds one, else None."""
    kind, path = mask_source(mask_directory)
    return path if kind == 'rtstruct' else None


def seg_in(mask_directory):
    """The path of the DICOM Segmentation file when `mask_source` finds one, else None."""
    kind, path = mask_source(mask_directory)
    return path if kind == 'seg' else None


def _n_files(volume):
    """The files a read volume came from: one per slice of a DICOM series, one NIfTI file."""
    return len(volume.frames) if isinstance(volume, dicom.DicomSeries) else 1


READERS = {'rtstruct': rtstruct, 'seg': seg}         # the kinds of `mask_source` that are one file, placed against the scan


class ImageDataset(torch.utils.data.Dataset):
    format = 'auto'             # the layout a class is bound to; the constructor's `format` overrides it
    files_read = 0              # files that `_load` has read in this process, over all datasets (`--cache_volumes` logs and resets it per epoch)

    def __init__(self, patient_directory, patient_key, mask_resample='auto', log_grids=True, format=None, mask_roi=None):
        if mask_resample not in MASK_RESAMPLE_MODES:
            raise ConfigurationError(f"mask_resample {mask_resample!r} is none of {MASK_RESAMPLE_MODES}")
        format = str(self.format if format is None else format).lower()
        if format not in FORMATS:
            raise ConfigurationError(f"format {format!r} is none of {FORMATS}")
        self.mask_resample = mask_resample
        self.mask_roi = mask_roi
        self._sources = {}                   # mask directory -> what `mask_source` found in it: (kind, path)
        self.patient_directory = str(patient_directory)
        self.patients = sorted(x for x in os.listdir(self.patient_directory)
                               if not x.startswith('.') and os.path.isdir(os.path.join(self.patient_directory, x)))
        self.patient_key = _read_key(patient_key)
        self.multimodal_identifier = 'image'
        self.transforms = None
        self.layout = self._detect_layout() if format == 'auto' else format
        for p in self.patients:
            if self._anon(p) not in self.patient_key:
                raise ConfigurationError(f"patient directory {p} ({self._anon(p)}) has no row in the patient key {patient_key}")
            self._files(p)
        # the headers alone: a mask on another grid needs both geometries, and is refused here rather than in the first epoch
        self.other_grid = [p for p in self.patients if self._check_grids(p, *(self._geometry(f) + (f,) for f in self._files(p)))]
        if log_grids and self.other_grid:
            logger.info("%d of %d patients under %s have a mask on another grid than the scan's: it is resampled into the scan's grid on the device",
                        len(self.other_grid), len(self.patients), self.patient_directory)

    def _detect_layout(self):
        """The one layout of the tree; a tree that mixes the two (or a patient directory that is neither) is refused."""
        found = {}
        for p in self.patients:
            found.setdefault(layout_of(os.path.join(self.patient_directory, p)), p)
        if None in found:
            raise ConfigurationError(f"patient directory {os.path.join(self.patient_directory, found[None])} holds neither a NIfTI scan* file "
                                     "nor the DICOM sub-directories image/ and mask/")
        if len(found) > 1:
            raise ConfigurationError(f"{self.patient_directory} mixes the two layouts: {found['nifti']} is NIfTI, {found['dicom']} is DICOM; "
                                     "one format per tree (Data.format forces one)")
        return next(iter(found), 'nifti')

    def _anon(self, patient):
        """The anonymised id of a patient directory: for DICOM the name itself when the key has it (upstream data/utils.py:8-14)."""
        if self.layout == 'dicom' and patient in self.patient_key:
            return patient
        return anon_id_of(patient)

    def _uid_of(self, patient):
        return self.patient_key[self._anon(patient)]

    def _geometry(self, path):
        """(extents, affine or None) from the headers alone.  An RTSTRUCT mask has no grid of its own: (None, None), once its ROI
        names have been read and `mask_roi` resolved against them (a bad name fails here, at construction).  So has a SEG mask
        until it is placed against its scan (`_check_grids`); its segment labels are resolved here as well."""
        kind, file = self._source(path)
        if kind in READERS:
            READERS[kind].resolve(READERS[kind].read(file, header_only=True), self.mask_roi)
            return None, None
        if self.layout == 'dicom':
            series = dicom.read_series(path, header_only=True)
            return series.shape, series.affine
        return nifti.read_geometry(path)

    def _source(self, path):
        """(kind, path) of a scan or mask: what `mask_source` finds in a mask/ directory of the DICOM layout, looked at once; image/
        directories and NIfTI files are always ('series', path)."""
        if self.layout != 'dicom' or os.path.basename(path) != 'mask':
            return 'series', path
        if path not in self._sources:
            self._sources[path] = mask_source(path)
        return self._sources[path]

    @property
    def uids(self):
        return [self._uid_of(p) for p in self.patients]

    def __len__(self):
        return len(self.patients)

    def _files(self, patient):
        d = os.path.join(self.patient_directory, patient)
        if self.layout == 'dicom':
            for sub in ('image', 'mask'):
                if not os.path.isdir(os.path.join(d, sub)):
                    raise ConfigurationError(f"patient {patient} (uid {self._uid_of(patient)}): no {sub}/ series directory in {d} (the DICOM layout; "
                                             "a NIfTI mask beside a DICOM scan is outside the path)")
            return os.path.join(d, 'image'), os.path.join(d, 'mask')
        files = sorted(f for f in os.listdir(d) if not f.startswith('.'))
        scans = [f for f in files if f.startswith('scan')]
        masks = [f for f in files if not f.startswith('scan')]
        if len(scans) != 1:
            raise ConfigurationError(f"patient {patient} (uid {self._uid_of(patient)}): {len(scans)} files named scan* in {d}, one expected")
        if len(masks) != 1:
            raise ConfigurationError(f"patient {patient} (uid {self._uid_of(patient)}): {'no mask' if not masks else 'several candidate masks'} beside {scans[0]} in {d}")
        return os.path.join(d, scans[0]), os.path.join(d, masks[0])

    def _load(self, patient):
        scan_path, mask_path = self._files(patient)
        read = dicom.read_series if self.layout == 'dicom' else nifti.read
        kind, file = self._source(mask_path)
        if kind in READERS:
            # the collate function places the frames of a SEG mask against the scan and unpacks them on the device; contours are born
            # on the scan's grid and rasterised there (no resample, no threshold)
            scan = read(scan_path)
            ImageDataset.files_read += _n_files(scan) + 1
            return scan, READERS[kind].select(READERS[kind].read(file), self.mask_roi)
        scan, mask = read(scan_path), read(mask_path)
        ImageDataset.files_read += _n_files(scan) + _n_files(mask)
        self._check_grids(patient, (scan.shape, scan.affine, scan_path), (mask.shape, mask.affine, mask_path))
        return scan, mask

    def _check_grids(self, patient, scan, mask):
        """scan, mask: (extents, affine or None, path).  True when the mask's extents differ from the scan's and can be resampled.
        An RTSTRUCT mask (extents None) is on the scan's grid by construction; its scan needs a geometry to place the contours by.
        A SEG mask (extents None as well) is placed here from its header: True when its frames form a grid of their own."""
        (sshape, saff, _), (mshape, maff, _) = scan, mask
        kind, path = self._source(mask[2])
        if kind in READERS and saff is None:
            raise ConfigurationError(f"patient {patient} (uid {self._uid_of(patient)}): {scan[2]} has no position / orientation to place the "
                                     f"{'frames' if kind == 'seg' else 'contours'} of {path} by")
        if kind == 'seg':
            place = seg.to_scan(seg.select(seg.read(path, header_only=True), self.mask_roi), sshape, saff)
            if not place.on_scan and self.mask_resample == 'never':
                raise ConfigurationError(f"patient {patient} (uid {self._uid_of(patient)}): scan extent {tuple(sshape)}, SEG extent {tuple(place.shape)}: "
                                         f"{path} is on a grid of its own (Data.mask_resample is 'never')")
            return not place.on_scan
        if kind == 'rtstruct':
            return False
        what = f"patient {patient} (uid {self._uid_of(patient)}): scan extent {tuple(sshape)}, mask extent {tuple(mshape)}"
        if len(sshape) != 3 or len(mshape) != 3:
            raise ConfigurationError(what)
        if tuple(sshape) == tuple(mshape):
            return False
        if self.mask_resample == 'never':
            raise ConfigurationError(what + " (Data.mask_resample is 'never')")
        geometry = "position / orientation" if self.layout == 'dicom' else "qform/sform"
        if saff is None and maff is None:
            raise ConfigurationError(what + f" and neither file has a {geometry} to resample by")
        if saff is None or maff is None:
            raise ConfigurationError(what + f" and {scan[2] if saff is None else mask[2]} has no {geometry} to resample by")
        return True

    def _index_of_uid(self, uid):
        for i, p in enumerate(self.patients):
            if self._uid_of(p) == int(uid):
                return i
        raise ConfigurationError(f"patient uid {uid} not found under {self.patient_directory}")

    def getDataByUID(self, uid):
        return self.__getitem__(self._index_of_uid(uid))


class _LabelledNifti(ImageDataset):
    survival = False

    def __init__(self, patient_directory, clinical_data, patient_key, slices=False, transforms=None, mask_resample='auto', log_grids=True,
                 format=None, mask_roi=None):
        super().__init__(patient_directory, patient_key, mask_resample, log_grids, format, mask_roi)
        if slices:
            raise ConfigurationError("slices=True (2-D slices of a volume) is outside the MI355X path")
        if transforms is not None:
            raise ConfigurationError("per-item transforms cannot run on raw voxels: pass --transforms (they act on the collated device batch)")
        self.labels = LabelTable(clinical_data)
        for p in self.patients:
            if self._uid_of(p) not in self.labels.row:
                raise ConfigurationError(f"patient {p} (uid {self._uid_of(p)}) has no row in the clinical csv {clinical_data}")

    def _volumes(self, patient):
        return [self._load(patient)]

    def __getitem__(self, index):
        patient = self.patients[index]
        uid = self._uid_of(patient)
        raw = RawPatient(uid, self._volumes(patient))
        if self.survival:
            return raw, self.labels.events(uid), self.labels.durations(uid)
        return raw, self.labels.events(uid)


class NiftiImageDataset(_LabelledNifti):
    """data/ImageDatasets.py:327-377: (image, label)."""


class NiftiSurvivalDataset(_LabelledNifti):
    """data/ImageDatasets.py:422-470: (image, events, durations)."""
    survival = True


class ImageClassificationDataset(_LabelledNifti):
    """data/ImageDatasets.py:224-292: (image, label) from the DICOM layout."""
    format = 'dicom'


class ImageSurvivalDataset(_LabelledNifti):
    """data/ImageDatasets.py:196-222: (image, events, durations) from the DICOM layout; masked like its classification twin (upstream
    returns the unmasked image there)."""
    format = 'dicom'
    survival = True


class _T1T2(_LabelledNifti):
    def __init__(self, t1_directory, t2_directory, clinical_data, patient_key, slices=False, transforms=None, mask_resample='auto', format=None,
                 mask_roi=None):
        cls = NiftiSurvivalDataset if self.survival else NiftiImageDataset
        self.t1_dataset = cls(t1_directory, clinical_data, patient_key, slices, None, mask_resample, format=format, mask_roi=mask_roi)
        self.t2_dataset = cls(t2_directory, clinical_data, patient_key, slices, None, mask_resample, format=format, mask_roi=mask_roi)
        if self.t1_dataset.layout != self.t2_dataset.layout:
            raise ConfigurationError(f"{t1_directory} is a {self.t1_dataset.layout} tree and {t2_directory} a {self.t2_dataset.layout} one: one format for both")
        super().__init__(t1_directory, clinical_data, patient_key, slices, transforms, mask_resample, log_grids=False,
                         format=self.t1_dataset.layout, mask_roi=mask_roi)   # (t1 has reported)
        self.t1_patients, self.t2_patients = self.t1_dataset.patients, self.t2_dataset.patients
        # patients common to both trees, by anonymised id; kept as the T1 directory names
        in_t2 = {self.t2_dataset._anon(p): p for p in self.t2_patients}
        self.patients = [p for p in self.t1_patients if self._anon(p) in in_t2]
        self._t2_of = {p: in_t2[self._anon(p)] for p in self.patients}

    def _volumes(self, patient):
        return [self.t1_dataset._load(patient), self.t2_dataset._load(self._t2_of[patient])]


class T1T2ImageDataset(_T1T2):
    """data/ImageDatasets.py:520-576: both modalities of the patients present in both trees, stacked along the channel axis."""


class T1T2SurvivalDataset(_T1T2):
    """data/ImageDatasets.py:578-640."""
    survival = True


class ImageDatasetByUIDs(torch.utils.data.Dataset):
    """data/ImageDatasets.py:310-325: the sub-dataset of `dataset` that can only reach the given uids."""

    def __init__(self, dataset, uids, seed=42, train_percent=0.8, transforms=None):
        self.dataset = dataset
        self.set_uids = [int(u) for u in uids]
        self.multimodal_identifier = getattr(dataset, 'multimodal_identifier', 'image')
        known = set(dataset.uids)
        missing = [u for u in self.set_uids if u not in known]
        if missing:
            raise ConfigurationError(f"uids {missing[:8]} are not in the dataset")

    @property
    def uids(self):
        return self.set_uids

    def getDataByUID(self, uid):
        return self.dataset.getDataByUID(uid)

    def __getitem__(self, index):
        return self.dataset.getDataByUID(self.set_uids[index])

    def __len__(self):
        return len(self.set_uids)
