"""Model factory of the reference's configuration layer (parser/parser.py:21-198), restricted to the fusion path.

`Parser(config).parseConfig()` reads the same YAML schema (config.yaml); `getModel(args)` builds the native DenseNet121 /
TinyDensenet and wraps it into `MultiModalModel` for `--images --preop|--postop` exactly like parser/parser.py:105-182.
Fixes: `--preop` alone yields the standalone clinical MLP; the predictor list may be given as an
integer count (`ClinicalModel.NUM_PREDICTORS`) for synthetic data.  `getImagePath()` / `getDatasets(args, image_path)` (parser.py:43-97,
184-198) build the local-disk image datasets from the `Data:` section (`image_loc`, `t1_path`, `t2_path`, `data_loc`, `key_loc`; the
command-line flags override it; `size: S`, 1..128, default 64, is the extent per axis the scans are ingested at -- `imageSize`;
`format: auto | nifti | dicom` names the patient directories' layout, detected per tree by default;
`mask_resample`, `mask_threshold` say what happens to a mask drawn on another grid than its scan's -- a DICOM mask is always resampled,
and binarised at 128 unless `mask_threshold` is set; `mask_roi` names the region of interest to take from an RTSTRUCT mask, which is
rasterised onto its scan's grid and takes neither resample nor threshold, or the segment to take, by its SegmentLabel, from a DICOM SEG
mask, which is unpacked onto its scan's grid when its frames lie on it and else resampled like a mask series).  DICOM means uncompressed single-frame series (`mmnn_sts_amd.data.dicom`); S3 and
segmentation datasets stay outside the path, and main.py substitutes synthetic patients when no image location is configured.
"""
import os

import yaml

from ..exceptions.exceptions import ConfigurationError, InitializationError
from ..data.ClinicalDatasets import ClinicalDataset
from ..data.ImageDatasets import NiftiImageDataset, NiftiSurvivalDataset, T1T2ImageDataset, T1T2SurvivalDataset
from ..data.MultiModalDatasets import MultiModalDataset, MultiModalSurvivalDataset
from ..models.densenet import DenseNet121, TinyDensenet
from ..models.mlp import MLP
from ..models.multimodal import MultiModalModel
from ..models.resnet import r3d_18

DEFAULT_CONFIG = {
    "ImageModel": {"name": "densenet121", "modality": "t1t2", "feature_layers": 12, "num_classes": 2, "spatial_dims": 3,
                   "in_channels": 2, "dropout_prob": 0.2},
    "ClinicalModel": {"PRE_OP_PREDICTORS": [f"predictor{i}" for i in range(32)], "POST_OP_PREDICTORS": []},
    "Hyperparameters": {"epochs": 100, "learning_rate": 5e-4, "momentum": 0.9, "weight_decay": 1e-4, "train_batch_size": 2,
                        "test_batch_size": 1, "seed": 42, "num_gpus": 1},
}


class Parser:
    def __init__(self, config_path=None):
        self.config_path = config_path
        self.config = None

    def parseConfig(self):
        if self.config_path is None:
            self.config = {k: dict(v) for k, v in DEFAULT_CONFIG.items()}
        else:
            with open(self.config_path) as f:
                self.config = yaml.safe_load(f)
        im = self.config['ImageModel']
        if im['modality'].lower().startswith('t1t2') and im['in_channels'] != 2:
            raise ConfigurationError('T1T2 ImageModel modality requires 2 input channels - current number of in_channels: {}'.format(im['in_channels']))
        return self.config

    def clinicalPredictors(self, args):
        cm = self.config['ClinicalModel']
        if 'NUM_PREDICTORS' in cm:
            return [f"predictor{i}" for i in range(int(cm['NUM_PREDICTORS']))]
        p = list(cm['PRE_OP_PREDICTORS'])
        if args.postop:
            p += list(cm.get('POST_OP_PREDICTORS', []))
        return p

    def predictors(self, args):
        """The columns of the tabular input: the clinical predictors; with --radiomics the feature columns of the radiomics csv -- alone,
        or behind the clinical ones when --preop / --postop is given too."""
        if not args.radiomics:
            return self.clinicalPredictors(args)
        clinical = self.clinicalPredictors(args) if (args.preop or args.postop) else []
        return clinical + self.radiomicsColumns()

    def radiomicsConfig(self):
        """`Radiomics: bin_width` (25), `max_bins` (256), `standardize` (true)."""
        rad = self.config.get('Radiomics') or {}
        try:
            out = {'bin_width': float(rad.get('bin_width', 25.0)), 'max_bins': int(rad.get('max_bins', 256)), 'standardize': bool(rad.get('standardize', True))}
        except (TypeError, ValueError):
            raise ConfigurationError('Radiomics.bin_width / max_bins {!r} / {!r} are not numbers'.format(rad.get('bin_width'), rad.get('max_bins')))
        if not (out['bin_width'] > 0.0 and out['bin_width'] < float('inf')) or not 1 <= out['max_bins'] <= 1024:
            raise ConfigurationError('Radiomics.bin_width must be positive and finite and max_bins within 1..1024, got {} and {}'.format(out['bin_width'], out['max_bins']))
        return out

    def radiomicsClasses(self):
        """`Radiomics: classes`: the texture classes extracted beside the default columns, a list drawn from glrlm, gldm, ngtdm (empty)."""
        from ..radiomics import texture_classes
        rad = self.config.get('Radiomics') or {}
        classes = rad.get('classes')
        if classes is not None and not isinstance(classes, (list, tuple, str)):
            raise ConfigurationError('Radiomics.classes must be a list drawn from glrlm, gldm, ngtdm, got {!r}'.format(classes))
        return texture_classes(classes)

    def radiomicsZones(self):
        """`Radiomics: glszm`: whether the 16 size-zone (GLSZM) columns are extracted behind the other classes (false)."""
        rad = self.config.get('Radiomics') or {}
        glszm = rad.get('glszm', False)
        if not isinstance(glszm, bool):
            raise ConfigurationError('Radiomics.glszm must be true or false, got {!r}'.format(glszm))
        return glszm

    def radiomicsMesh(self):
        """`Radiomics: mesh_shape`: whether the 8 mesh-based shape columns are extracted behind all the others (false)."""
        rad = self.config.get('Radiomics') or {}
        mesh = rad.get('mesh_shape', False)
        if not isinstance(mesh, bool):
            raise ConfigurationError('Radiomics.mesh_shape must be true or false, got {!r}'.format(mesh))
        return mesh

    def radiomicsLog(self, sigma=None, bin_width=None):
        """`Radiomics: log: {sigma: [1.0, 3.0], bin_width: 25}`: the Laplacian-of-Gaussian image type -> {'sigma': the scales in mm,
        de-duplicated and ascending (empty: no filtered image), 'bin_width': the filtered images' bin width (`Radiomics: bin_width` when
        not given)}.  `sigma` / `bin_width`: a command line's values, which go before the config's."""
        from ..radiomics import log_sigmas
        log = (self.config.get('Radiomics') or {}).get('log')
        valid = 'Radiomics.log must be a mapping of `sigma` (a list of positive finite numbers, in mm) and optionally `bin_width` (a positive finite number)'
        if log is None:
            log = {}
        if not isinstance(log, dict) or set(log) - {'sigma', 'bin_width'}:
            raise ConfigurationError('{}, got {!r}'.format(valid, log))
        if 'sigma' in log and not isinstance(log['sigma'], (list, tuple)):
            raise ConfigurationError('{}, got sigma {!r}'.format(valid, log['sigma']))
        sigmas = log_sigmas(sigma if sigma is not None else log.get('sigma'))
        bw = bin_width if bin_width is not None else log.get('bin_width', self.radiomicsConfig()['bin_width'])
        if isinstance(bw, bool) or not isinstance(bw, (int, float)) or not (bw > 0.0 and bw < float('inf')):
            raise ConfigurationError('{}, got bin_width {!r}'.format(valid, bw))
        return {'sigma': sigmas, 'bin_width': float(bw)}

    def radiomicsNormalize(self, flag=False, scale=None, outliers=None):
        """`Radiomics: normalize: true | {scale: 100, outliers: 3}`: the whole-scan intensity normalisation ahead of the extraction ->
        None (off, the default) or (scale, outliers).  `flag` / `scale` / `outliers`: a command line's values, which go before the
        config's; any of them switches the step on.  The default scale is 100, not PyRadiomics' 1, because of the default bin width 25."""
        from ..radiomics import normalize_settings
        norm = (self.config.get('Radiomics') or {}).get('normalize')
        if norm is not None and not isinstance(norm, (bool, dict)):
            raise ConfigurationError('Radiomics.normalize must be true / false or a mapping of `scale` and `outliers`, got {!r}'.format(norm))
        settings = dict(norm) if isinstance(norm, dict) else {}
        if scale is not None:
            settings['scale'] = scale
        if outliers is not None:
            settings['outliers'] = outliers
        on = bool(flag) or scale is not None or outliers is not None or isinstance(norm, dict) or norm is True
        return normalize_settings(settings) if on else None

    def radiomicsResample(self, spacing=None):
        """`Radiomics: resample: {spacing: [1, 1, 1]}` (or one number): the voxel spacing in mm scan and mask are resampled to ahead of
        the extraction -> None (off, the default) or the three spacings; 0 keeps an axis.  `spacing`: a command line's value, which goes
        before the config's."""
        from ..radiomics import resample_spacing
        res = (self.config.get('Radiomics') or {}).get('resample')
        if spacing is not None:
            return resample_spacing(spacing)
        if res is not None and not isinstance(res, dict):
            raise ConfigurationError('Radiomics.resample must be a mapping of `spacing` (one number or three, in mm), got {!r}'.format(res))
        if isinstance(res, dict) and isinstance(res.get('spacing'), str):
            raise ConfigurationError('Radiomics.resample.spacing must be one number or a list of three (mm), got {!r}'.format(res['spacing']))
        return resample_spacing(res)

    def radiomicsShell(self, shell_mm=None):
        """`Radiomics: shell_mm: [5, 10]`: the widths in mm of the peritumoural shells whose features follow every `original_*` and
        `log-*` column -> the widths, de-duplicated and ascending (empty, the default: no shell).  `shell_mm`: a command line's value
        (`--shell_mm 5,10`), which goes before the config's."""
        from ..radiomics import shell_widths
        value = (self.config.get('Radiomics') or {}).get('shell_mm')
        if shell_mm is None and isinstance(value, str):
            raise ConfigurationError('Radiomics.shell_mm must be a list of positive finite numbers (mm), got {!r}'.format(value))
        return shell_widths(shell_mm if shell_mm is not None else value)

    def radiomicsExtraction(self, args):
        """What the extraction of a radiomics table is run with -> the keyword arguments of `radiomics.extract_modalities` behind its
        datasets and device: the two bin settings, the mask threshold (`Data: mask_threshold`; None: each scan's default) and the
        switches of `radiomics.extract`.  `args`: the flags of `radiomics.add_extraction_arguments`, which go before the config's
        `Radiomics:` section; `classes` / `glszm` are read when the command line has them (the tool's alone)."""
        from ..radiomics import texture_classes
        rc = self.radiomicsConfig()
        classes = texture_classes(args.classes) if getattr(args, 'classes', None) is not None else self.radiomicsClasses()
        glszm = getattr(args, 'glszm', False) or self.radiomicsZones()
        mesh = args.mesh_shape or self.radiomicsMesh()
        log = self.radiomicsLog(args.log_sigma, args.log_bin_width)
        normalize = self.radiomicsNormalize(args.normalize, args.normalize_scale, args.normalize_outliers)
        resample = self.radiomicsResample(args.resample_spacing)
        shells = self.radiomicsShell(args.shell_mm)
        threshold = (self.config.get('Data') or {}).get('mask_threshold')
        return dict(bin_width=rc['bin_width'], max_bins=rc['max_bins'], mask_threshold=None if threshold is None else float(threshold),
                    classes=classes, glszm=glszm, mesh=mesh, log_sigma=log['sigma'], log_bin_width=log['bin_width'], normalize=normalize,
                    resample=resample, shell_mm=shells)

    def maskMargin(self, flag=None):
        """`Data: mask_margin_mm`: the margin in mm every mask is dilated by on the device ahead of the scan ingest -> None (off, the
        default) or a positive finite number.  `flag`: the command line's `--mask_margin_mm`, which goes before the config's."""
        from ..data.ingest import margin_radius
        value = flag if flag is not None else (self.config.get('Data') or {}).get('mask_margin_mm')
        return margin_radius(value, '--mask_margin_mm' if flag is not None else 'Data.mask_margin_mm')

    def _radiomicsExcluded(self):
        rm = self.config.get('RadiomicsModel') or {}
        return list(rm.get('RADIOMICS_EXCLUDE_COLUMNS') or []), list(rm.get('RADIOMICS_LABEL_COLUMNS') or [])

    def radiomicsColumns(self):
        """The feature columns of `Data: rad_loc`, from its header alone."""
        from ..data.RadiomicsDatasets import feature_columns
        with open(self._data('rad_loc')) as f:
            header = [c.strip() for c in f.readline().strip().split(',')]
        exclude, label = self._radiomicsExcluded()
        return feature_columns(header, exclude + label)

    def applyDataFlags(self, args):
        """The `Data:` section with --image_loc / --data_loc / --key_loc laid over it (t1_path / t2_path default to 't1' / 't2')."""
        data = dict(self.config.get('Data') or {})
        for k in ('image_loc', 'data_loc', 'key_loc', 'rad_loc'):
            if getattr(args, k, None):
                data[k] = getattr(args, k)
        data.setdefault('t1_path', 't1')
        data.setdefault('t2_path', 't2')
        self.config['Data'] = data
        return data

    def _data(self, key):
        value = (self.config.get('Data') or {}).get(key)
        if not value:
            raise ConfigurationError('Data.{0} is not configured (config `Data: {0}:` or --{0})'.format(key))
        return value

    def maskResample(self):
        """(`Data: mask_resample`, `Data: mask_threshold`), defaults ('auto', 0.5); the threshold's default is 128 (upstream's
        `mask > 128`) once `getDatasets` has found the image tree to be in the DICOM layout.  'auto': a mask whose extents differ from its scan's
        is resampled into the scan's grid on the device (both files need a qform / sform), equal extents are multiplied voxelwise;
        'geometry': also resampled when equal extents sit elsewhere in space (a corner of the scan grid maps more than 1e-3 voxel away
        from itself); 'never': differing extents are refused.  The threshold binarises the interpolated mask: 0.5 for 0/1 masks, 128
        (upstream's value) for 0/255 masks."""
        from ..data.ingest import DICOM_MASK_THRESHOLD, MASK_RESAMPLE_MODES, NIFTI_MASK_THRESHOLD
        data = self.config.get('Data') or {}
        mode = str(data.get('mask_resample', 'auto')).lower()
        if mode not in MASK_RESAMPLE_MODES:
            raise ConfigurationError('Data.mask_resample {!r} is none of {}'.format(data.get('mask_resample'), ', '.join(MASK_RESAMPLE_MODES)))
        try:
            default = DICOM_MASK_THRESHOLD if getattr(self, 'image_layout', 'nifti') == 'dicom' else NIFTI_MASK_THRESHOLD
            threshold = float(default if data.get('mask_threshold') is None else data['mask_threshold'])
        except (TypeError, ValueError):
            threshold = float('nan')
        if threshold != threshold or threshold in (float('inf'), float('-inf')):
            raise ConfigurationError('Data.mask_threshold {!r} is not a finite number'.format(data.get('mask_threshold')))
        return mode, threshold

    def maskRoi(self):
        """`Data: mask_roi`: the ROIName to take from a mask that is an RT Structure Set, or the SegmentLabel to take from one that is a
        DICOM SEG file (exact, case-insensitive), or None (the default: the file's only ROI / segment).  The datasets resolve it against every patient's file when they are built."""
        value = (self.config.get('Data') or {}).get('mask_roi')
        if value is None:
            return None
        if not isinstance(value, str) or not value.strip():
            raise ConfigurationError('Data.mask_roi {!r} is not a ROI name (a non-empty string)'.format(value))
        return value.strip()

    def minImageSize(self):
        """The smallest cubic input extent at which the native plan (csrc/densenet.hip: plan_build) still leaves the last dense block of
        the configured DenseNet a voxel: the stem and the pool halve the extent rounding up, every transition halves it rounding down.
        1 for a model that is no DenseNet (r3d_18 pools adaptively)."""
        name = self.config['ImageModel']['name'].lower()
        blocks = 4 if name.startswith('densenet121') else 3 if name.startswith('tinydensenet') else 0
        if not blocks:
            return 1
        size = 1
        while (((size - 1) // 2) // 2 + 1) >> (blocks - 1) < 1:
            size += 1
        return size

    def imageSize(self, flag=None):
        """`Data: size`: the extent S per axis that the scan ingest, the `--transforms` Resize and the exports work at -> an integer in
        1..128, default 64 (upstream's Resize((64,64,64))).  `flag`: the command line's `--image_size`, which goes before the config's."""
        from ..data.ingest import MAX_SIZE, SIZE
        value = flag if flag is not None else (self.config.get('Data') or {}).get('size', SIZE)
        where = '--image_size' if flag is not None else 'Data.size'
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= MAX_SIZE:
            raise ConfigurationError('{} {!r} is not an integer in 1..{}'.format(where, value, MAX_SIZE))
        lowest = self.minImageSize()
        if value < lowest:
            raise ConfigurationError('{} {} is within 1..{} but leaves the last dense block of {} no voxel: its smallest extent is {}'.format(
                where, value, MAX_SIZE, self.config['ImageModel']['name'], lowest))
        return value

    def dataFormat(self):
        """`Data: format`: 'auto' (the default: the layout is detected per tree), 'nifti' or 'dicom'."""
        from ..data.ImageDatasets import FORMATS
        value = str((self.config.get('Data') or {}).get('format') or 'auto').lower()
        if value not in FORMATS:
            raise ConfigurationError('Data.format {!r} is none of {}'.format((self.config.get('Data') or {}).get('format'), ', '.join(FORMATS)))
        return value

    def getImagePath(self):
        """parser/parser.py:184-198: the modality's directory under image_loc; a (t1, t2) tuple for 't1t2'."""
        modality = self.config['ImageModel']['modality'].lower()
        if modality.startswith('t1t2'):
            return (os.path.join(self._data('image_loc'), self._data('t1_path')), os.path.join(self._data('image_loc'), self._data('t2_path')))
        if modality.startswith('t1'):
            return os.path.join(self._data('image_loc'), self._data('t1_path'))
        if modality.startswith('t2'):
            return os.path.join(self._data('image_loc'), self._data('t2_path'))
        raise ConfigurationError("ImageModel modality {!r} is none of 't1', 't2', 't1t2'".format(self.config['ImageModel']['modality']))

    def getDatasets(self, args, image_path=None):
        """parser/parser.py:43-97 for the local-disk cases: the clinical dataset (with --preop / --postop), the image dataset of
        the modality (with --images; NIfTI or DICOM layout, see `Data: format`), and their MultiModal(Survival)Dataset when both are asked for."""
        if not (args.classification or args.survival):
            raise ConfigurationError('getDatasets needs --survival or --classification to pick the dataset classes')
        datasets = []
        if args.preop or args.postop:
            datasets.append(ClinicalDataset(self._data('data_loc'), self.clinicalPredictors(args), classification=args.classification, survival=args.survival))
        if getattr(args, 'radiomics', False):       # (the image tests build their arguments without the field)
            from ..data.RadiomicsDatasets import JoinedTableDataset, RadiomicsClassificationDataset, RadiomicsSurvivalDataset
            cls = RadiomicsSurvivalDataset if args.survival else RadiomicsClassificationDataset
            self.radiomics_dataset = cls(self._data('rad_loc'), self._data('data_loc'), *self._radiomicsExcluded())
            datasets.append(self.radiomics_dataset)
            if len(datasets) == 2:       # clinical and radiomic columns of one patient are one predictor table, clinical first
                datasets = [JoinedTableDataset(datasets)]
        if args.images:
            both = isinstance(image_path, tuple)
            if args.survival:
                cls = T1T2SurvivalDataset if both else NiftiSurvivalDataset
            else:
                cls = T1T2ImageDataset if both else NiftiImageDataset
            paths = image_path if both else (image_path,)
            datasets.append(cls(*paths, self._data('data_loc'), self._data('key_loc'), mask_resample=self.maskResample()[0],
                                format=self.dataFormat(), mask_roi=self.maskRoi()))
            self.image_layout = datasets[-1].layout
        if len(datasets) == 1:
            return datasets[0]
        return MultiModalSurvivalDataset(datasets) if args.survival else MultiModalDataset(datasets)

    def getModel(self, args):
        if self.config is None:
            raise InitializationError('Attempted to load model prior to parsing config parameters, config must be parsed prior to loading model')
        im = self.config['ImageModel']
        name = im['name'].lower()
        clinical = args.preop or args.postop or args.radiomics
        if not args.images and clinical:
            return MLP(len(self.predictors(args)), im['num_classes'], im['feature_layers'])
        kw = dict(spatial_dims=im['spatial_dims'], in_channels=im['in_channels'], out_channels=im['num_classes'],
                  feature_channels=im['feature_layers'], dropout_prob=im['dropout_prob'])
        if name.startswith('densenet121'):
            model = DenseNet121(**kw)
        elif name.startswith('tinydensenet'):
            model = TinyDensenet(**kw)
        elif name.startswith('r3d_18'):
            model = r3d_18(im['num_classes'])                       # parser/parser.py:151-152
        else:
            raise ConfigurationError('Model name not recognized: {}\n\tThe MI355X path provides densenet121, tinydensenet and r3d_18'.format(name))
        if args.images and clinical:
            # parser/parser.py:159-160,171-172: only encoders with .backbone / .features can feed the fusion model
            assert name.startswith('tinydensenet') or name.startswith('densenet121'), \
                "Image models used to build multimodal models must be one of 'tinydensenet' or 'densenet121'"
            model = MultiModalModel(model, self.predictors(args), im['num_classes'], im['feature_layers'], blend=args.blend)
        return model
