"""Every exit `main.main(argv)` can reach without a device, with its full message, and which message wins when an argv breaks two rules:
the checks run in one order, and that order is part of the command line's behaviour.  The messages were recorded from the command line
as it stood before the checks were gathered into `resolve_settings`.  Valid argv of each mode end at the device check."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import main as M  # noqa: E402
from tests._cli import tiny_config  # noqa: E402

NO_DEVICE = "mmnn_sts_amd runs on the MI355X only (no CPU path)"
TREE = ["--image_loc", "{tmp}/tree", "--key_loc", "{tmp}/key.csv", "--data_loc", "{tmp}/clinical.csv"]
RAD = ["--radiomics", "--rad_loc", "{tmp}/rad.csv", "--data_loc", "{tmp}/clinical.csv"]
T1 = dict(modality="t1", in_channels=1)

# (id, argv, tiny_config's keywords or None for no --config, environment, the message)
ROWS = [
    ("segmentation", ["--segmentation"], None, {}, "--segmentation is outside the MI355X fusion path (SURVEY 2)"),
    ("lr_finder needs images classification", ["--lr_finder", "--images", "--survival"], None, {},
     "--lr_finder runs upstream's find_lr on an image classification dataset: it needs --images --classification and no clinical flags "
     "(--preop / --postop)"),
    ("lr_finder with preop", ["--lr_finder", "--images", "--classification", "--preop"], None, {},
     "--lr_finder runs upstream's find_lr on an image classification dataset: it needs --images --classification and no clinical flags "
     "(--preop / --postop)"),
    ("lr_finder two ranks", ["--lr_finder", "--images", "--classification"], None, {"WORLD_SIZE": "2"},
     "--lr_finder is single-process (as upstream's find_lr); run it without torch.distributed.run"),
    ("bootstrap in training", ["--bootstrap", "--images", "--survival"], None, {},
     "--bootstrap resamples the evaluation of `--inference --survival` (main.py:767-887); it has no meaning for training runs"),
    ("occlusion alone", ["--occlusion", "--preop", "--survival"], None, {},
     "--occlusion writes occlusion sensitivity maps of the image input at inference: it needs --inference and --images"),
    ("occlusion without images", ["--occlusion", "--inference", "--preop", "--survival"], None, {},
     "--occlusion writes occlusion sensitivity maps of the image input at inference: it needs --images"),
    ("occlusion with bootstrap", ["--occlusion", "--inference", "--images", "--survival", "--bootstrap"], None, {},
     "--occlusion excludes --bootstrap (bootstrapping writes no maps, main.py:774-777)"),
    ("occlusion stride", ["--occlusion", "--inference", "--images", "--survival", "--occlusion_stride", "20"], None, {},
     "--occlusion needs 1 <= --occlusion_stride (20) <= --occlusion_window (16) and --occlusion_batch (8) >= 1"),
    ("transforms without images", ["--transforms", "--preop", "--classification"], None, {}, "--transforms acts on image volumes: it needs --images"),
    ("radiomics without a table", ["--radiomics", "--survival"], None, {},
     "--radiomics needs --rad_loc (a csv of radiomic features with the column MRN) or --image_loc (patient directories to extract the "
     "features from)"),
    ("radiomics extraction on two ranks", ["--radiomics", "--survival", *TREE], None, {"WORLD_SIZE": "2"},
     "--radiomics without --rad_loc extracts the features in a single process: run the extraction once (python -m mmnn_sts_amd.radiomics) "
     "and pass its csv as --rad_loc"),
    ("radiomics csv without clinical", ["--radiomics", "--survival", "--rad_loc", "{tmp}/rad.csv"], None, {},
     "--radiomics needs --data_loc (the clinical csv with uid, event{i}, duration{i})"),
    ("radiomics tree without key and clinical", ["--radiomics", "--survival", "--image_loc", "{tmp}/tree"], None, {},
     "--radiomics needs --data_loc and --key_loc (the clinical csv with uid, event{i}, duration{i}; the patient key csv with the columns "
     "'Anon MRN', 'MRN')"),
    ("radiomics images without tree", [*RAD, "--images", "--survival"], None, {},
     "--radiomics with --images pairs each patient's features with their scans: it needs --image_loc"),
    ("cache_gb alone", ["--cache_gb", "2", "--images", "--survival"], None, {}, "--cache_gb is the budget of the volume cache: it needs --cache_volumes"),
    ("cache_gb in config alone", ["--images", "--survival"], dict(data={"cache_gb": 2}), {},
     "--cache_gb is the budget of the volume cache: it needs --cache_volumes"),
    ("cache without tree", ["--cache_volumes", "--images", "--survival"], None, {},
     "--cache_volumes keeps the ingested scans of patient directories on the device: it needs --image_loc"),
    ("cache in config without tree", ["--images", "--survival"], dict(data={"cache": True}), {},
     "--cache_volumes keeps the ingested scans of patient directories on the device: it needs --image_loc"),
    ("cache at inference", ["--cache_volumes", "--inference", "--images", "--survival", *TREE], None, {},
     "--cache_volumes saves the re-reading of patients in later epochs: --inference reads each patient once, run it without"),
    ("cache budget not positive", ["--cache_volumes", "--cache_gb", "-1", "--images", "--survival", *TREE], None, {},
     "--cache_gb -1.0 is not a positive number of GB"),
    ("cache budget in config not a number", ["--cache_volumes", "--images", "--survival", *TREE], dict(data={"cache_gb": "many"}), {},
     "--cache_gb 'many' is not a positive number of GB"),
    ("mask margin not positive", ["--mask_margin_mm", "-1", "--images", "--survival", *TREE], None, {}, '--mask_margin_mm must be a positive finite number of mm, got -1.0'),
    ("mask margin in config not a number", ["--images", "--survival", *TREE], dict(data={"mask_margin_mm": "wide"}), {}, "Data.mask_margin_mm must be a positive finite number of mm, got 'wide'"),
    ("shell widths not numbers", ["--shell_mm", "a,b", "--radiomics", "--survival", *TREE], None, {}, "radiomics: shell width 'a' is not a positive finite number (mm)"),
    ("shell widths in config a string", ["--radiomics", "--survival", *TREE], dict(radiomics={"shell_mm": "5,10"}), {}, "Radiomics.shell_mm must be a list of positive finite numbers (mm), got '5,10'"),
    ("mask margin without tree", ["--mask_margin_mm", "5", "--images", "--survival"], None, {},
     "--mask_margin_mm / `Data: mask_margin_mm` widens the masks of patient directories: it needs --image_loc (synthetic patients have no "
     "mask)"),
    ("shell flag with a table", ["--shell_mm", "5", *RAD, "--survival"], None, {},
     "--shell_mm adds columns to the table extracted on the device: it needs --radiomics and no --rad_loc"),
    ("shell flag without radiomics", ["--shell_mm", "5", "--images", "--survival"], None, {},
     "--shell_mm adds columns to the table extracted on the device: it needs --radiomics and no --rad_loc"),
    ("tree without images", ["--preop", "--survival", *TREE], None, {}, "--image_loc points at NIfTI patient directories: it needs --images"),
    ("tree without key", ["--images", "--survival", "--image_loc", "{tmp}/tree", "--data_loc", "{tmp}/clinical.csv"], None, {},
     "--image_loc needs --key_loc (the patient key csv with the columns 'Anon MRN', 'MRN'; the clinical csv with uid, predictors, event{i}, "
     "duration{i})"),
    ("tree without key and clinical", ["--images", "--survival", "--image_loc", "{tmp}/tree"], None, {},
     "--image_loc needs --key_loc and --data_loc (the patient key csv with the columns 'Anon MRN', 'MRN'; the clinical csv with uid, "
     "predictors, event{i}, duration{i})"),
    ("lr_finder on a tree", ["--lr_finder", "--images", "--classification", *TREE], None, {},
     "--lr_finder runs on synthetic patients: run it without --image_loc"),
    ("channels against modality", ["--images", "--survival", *TREE], dict(modality="t1", in_channels=2), {},
     "ImageModel modality t1 yields 1 channel(s) per patient, in_channels is 2"),
    ("scan_space in training", ["--scan_space", "--images", "--survival", *TREE], None, {},
     "--scan_space lays the Grad-CAM attention maps over the patients' scans: it needs --inference, --image_loc (NIfTI patient directories) "
     "and Grad-CAM on (--images, neither --no_gradcam nor --bootstrap)"),
    ("scan_space without tree", ["--scan_space", "--inference", "--images", "--survival"], None, {},
     "--scan_space lays the Grad-CAM attention maps over the patients' scans: it needs --inference, --image_loc (NIfTI patient directories) "
     "and Grad-CAM on (--images, neither --no_gradcam nor --bootstrap)"),
    ("image_size without images", ["--image_size", "32", "--preop", "--survival"], None, {},
     "--image_size / `Data: size` is the extent of the image volumes: it needs --images"),
    ("size in config without images", ["--preop", "--survival"], dict(data={"size": 32}), {},
     "--image_size / `Data: size` is the extent of the image volumes: it needs --images"),
    ("image_size out of range", ["--image_size", "200", "--images", "--survival"], None, {}, '--image_size 200 is not an integer in 1..128'),
    ("image_size below the model's", ["--image_size", "8", "--images", "--survival"], None, {}, '--image_size 8 is within 1..128 but leaves the last dense block of densenet121 no voxel: its smallest extent is 29'),
    ("size in config not an integer", ["--images", "--survival"], dict(data={"size": 32.5}), {}, 'Data.size 32.5 is not an integer in 1..128'),
    # ---- two rules broken: which message wins -------------------------------------------------------------------------------------
    ("cache_gb alone before the missing key", ["--cache_gb", "2", "--images", "--survival", "--image_loc", "{tmp}/tree", "--data_loc", "{tmp}/clinical.csv"],
     None, {}, "--cache_gb is the budget of the volume cache: it needs --cache_volumes"),
    ("scan_space without Grad-CAM, occlusion in order", ["--occlusion", "--scan_space", "--no_gradcam", "--inference", "--images", "--survival", *TREE], None, {},
     "--scan_space lays the Grad-CAM attention maps over the patients' scans: it needs --inference, --image_loc (NIfTI patient directories) "
     "and Grad-CAM on (--images, neither --no_gradcam nor --bootstrap)"),
    ("occlusion stride before scan_space", ["--occlusion", "--occlusion_stride", "0", "--scan_space", "--no_gradcam", "--inference", "--images", "--survival", *TREE],
     None, {}, "--occlusion needs 1 <= --occlusion_stride (0) <= --occlusion_window (16) and --occlusion_batch (8) >= 1"),
    ("lr_finder with radiomics", ["--lr_finder", "--images", "--classification", *RAD, "--image_loc", "{tmp}/tree", "--key_loc", "{tmp}/key.csv"], None, {},
     "--lr_finder runs on synthetic image patients: run it without --radiomics"),
    ("lr_finder with radiomics and no tree", ["--lr_finder", "--images", "--classification", *RAD], None, {},
     "--radiomics with --images pairs each patient's features with their scans: it needs --image_loc"),
    ("transforms before image_size", ["--image_size", "8", "--transforms", "--preop", "--survival"], None, {},
     "--transforms acts on image volumes: it needs --images"),
    ("bootstrap before cache", ["--bootstrap", "--cache_volumes", "--images", "--survival"], None, {},
     "--bootstrap resamples the evaluation of `--inference --survival` (main.py:767-887); it has no meaning for training runs"),
    ("cache before mask margin", ["--cache_volumes", "--mask_margin_mm", "-1", "--images", "--survival"], None, {},
     "--cache_volumes keeps the ingested scans of patient directories on the device: it needs --image_loc"),
    ("mask margin value before its tree", ["--mask_margin_mm", "-1", "--images", "--survival"], None, {}, '--mask_margin_mm must be a positive finite number of mm, got -1.0'),
    ("shell value before its mode", ["--shell_mm", "a", "--images", "--survival"], None, {}, "radiomics: shell width 'a' is not a positive finite number (mm)"),
    ("missing key before scan_space", ["--scan_space", "--images", "--survival", "--image_loc", "{tmp}/tree"], None, {},
     "--image_loc needs --key_loc and --data_loc (the patient key csv with the columns 'Anon MRN', 'MRN'; the clinical csv with uid, "
     "predictors, event{i}, duration{i})"),
    ("scan_space before image_size", ["--scan_space", "--image_size", "200", "--images", "--survival"], None, {},
     "--scan_space lays the Grad-CAM attention maps over the patients' scans: it needs --inference, --image_loc (NIfTI patient directories) "
     "and Grad-CAM on (--images, neither --no_gradcam nor --bootstrap)"),
    # ---- valid argv of each mode: the first thing missing is the device -----------------------------------------------------------
    ("tabular classification", ["--preop", "--classification"], {}, {}, NO_DEVICE),
    ("tabular inference of a csv", ["--inference", "--preop", "--survival", "--data_loc", "{tmp}/clinical.csv"], {}, {}, NO_DEVICE),
    ("image-only survival", ["--images", "--survival", "--transforms", "--image_size", "32"], T1, {}, NO_DEVICE),
    ("fusion with the blender", ["--images", "--preop", "--survival", "--blend"], {}, {}, NO_DEVICE),
    ("tree training", ["--images", "--preop", "--survival", "--cache_volumes", "--cache_gb", "2", "--transforms", "--mask_margin_mm", "5", *TREE], {}, {},
     NO_DEVICE),
    ("tree inference", ["--inference", "--images", "--preop", "--survival", "--scan_space", "--occlusion", *TREE], {}, {}, NO_DEVICE),
    ("lr_finder", ["--lr_finder", "--images", "--classification"], T1, {}, NO_DEVICE),
    ("radiomics table", [*RAD, "--survival"], {}, {}, NO_DEVICE),
    ("radiomics table behind clinical columns", [*RAD, "--preop", "--classification"], {}, {}, NO_DEVICE),
    ("radiomics extraction", ["--radiomics", "--survival", "--shell_mm", "5", "--log_sigma", "1,3", *TREE], {}, {}, NO_DEVICE),
    ("radiomics fusion on a tree", [*RAD, "--images", "--survival", "--image_loc", "{tmp}/tree", "--key_loc", "{tmp}/key.csv"], {}, {}, NO_DEVICE),
]


def run_row(tmp_path, monkeypatch, argv, config, env):
    """The exit message of `main.main` for a row; None when it returned."""
    (tmp_path / "rad.csv").write_text("MRN,original_firstorder_Mean,original_shape_VoxelVolume\n1,0.5,8.0\n")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = [a.replace("{tmp}", str(tmp_path)) for a in argv] + ["--output_path", str(tmp_path / "out")]
    if config is not None:
        argv += ["--config", tiny_config(tmp_path, **config)]
    try:
        M.main(argv)
    except SystemExit as e:
        return str(e)
    return None


@pytest.mark.parametrize("argv,config,env,message", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_the_exit_and_its_message(tmp_path, monkeypatch, argv, config, env, message):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert run_row(tmp_path, monkeypatch, argv, config, env) == message
