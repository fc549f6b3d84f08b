"""The settings of a radiomics extraction are resolved once (`Parser.radiomicsExtraction`): for the same flags and config, `main.py
--radiomics` without `--rad_loc` and `python -m mmnn_sts_amd.radiomics` hand `extract_modalities` the same keyword arguments, and
with everything off those are the defaults of `extract`."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import main as M  # noqa: E402
from mmnn_sts_amd import radiomics  # noqa: E402
from tests._cli import tiny_config  # noqa: E402

ALL_OFF = dict(bin_width=25.0, max_bins=256, mask_threshold=None, classes=(), glszm=False, mesh=False, log_sigma=(), log_bin_width=25.0,
               normalize=None, resample=None, shell_mm=())
SECTIONS = {
    "no section": None,
    "bins": {"bin_width": 10, "max_bins": 64},
    "classes": {"classes": ["ngtdm", "glrlm"]},
    "glszm": {"glszm": True},
    "mesh": {"mesh_shape": True},
    "log": {"log": {"sigma": [3.0, 1.0], "bin_width": 5}},
    "normalize": {"normalize": {"scale": 50, "outliers": 3}},
    "resample": {"resample": {"spacing": [1, 1, 2]}},
    "shell": {"shell_mm": [10, 5]},
    "all": {"bin_width": 10, "max_bins": 64, "classes": ["gldm"], "glszm": True, "mesh_shape": True, "log": {"sigma": [2.0]}, "normalize": True,
            "resample": {"spacing": 1.5}, "shell_mm": [4]},
}
FLAGS = {
    "no flag": [],
    "mesh": ["--mesh_shape"],
    "log": ["--log_sigma", "1,3", "--log_bin_width", "7.5"],
    "normalize": ["--normalize_scale", "20"],
    "resample": ["--resample_spacing", "2,2,2"],
    "shell": ["--shell_mm", "6,3"],
    "all": ["--mesh_shape", "--log_sigma", "0.5", "--log_bin_width", "2", "--normalize", "--normalize_outliers", "2.5", "--resample_spacing", "1,1,1",
            "--shell_mm", "8"],
}
# what the rows whose outcome is plain to see must give
EXPECTED = {
    ("no section", "no flag"): ALL_OFF,
    ("all", "no flag"): dict(bin_width=10.0, max_bins=64, mask_threshold=0.25, classes=("gldm",), glszm=True, mesh=True, log_sigma=(2.0,),
                             log_bin_width=10.0, normalize=(100.0, 0.0), resample=(1.5, 1.5, 1.5), shell_mm=(4.0,)),
    ("all", "all"): dict(bin_width=10.0, max_bins=64, mask_threshold=0.25, classes=("gldm",), glszm=True, mesh=True, log_sigma=(0.5,),
                         log_bin_width=2.0, normalize=(100.0, 2.5), resample=(1.0, 1.0, 1.0), shell_mm=(8.0,)),
    ("no section", "shell"): dict(ALL_OFF, shell_mm=(3.0, 6.0)),
}


@pytest.fixture
def captured(monkeypatch):
    calls = []
    monkeypatch.setattr(radiomics, "tree_datasets", lambda parser, directories, key_loc: list(directories))
    monkeypatch.setattr(radiomics, "extract_modalities", lambda sets, device, *args, **kw: calls.append((len(sets), args, kw)) or [])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)           # (the extraction's own device check; nothing is launched)
    return calls


@pytest.mark.parametrize("flags", FLAGS, ids=list(FLAGS))
@pytest.mark.parametrize("section", SECTIONS, ids=list(SECTIONS))
def test_both_command_lines_resolve_the_same_settings(tmp_path, captured, section, flags):
    for m in ("t1", "t2"):
        (tmp_path / "tree" / m).mkdir(parents=True)
    cfg = tiny_config(tmp_path, radiomics=SECTIONS[section], data={"mask_threshold": 0.25} if section == "all" else None)
    loc = ["--config", cfg, "--image_loc", str(tmp_path / "tree"), "--key_loc", str(tmp_path / "key.csv")]
    radiomics.main([*loc, "--out", str(tmp_path / "tool.csv"), *FLAGS[flags]])
    a = M.build_arg_parser().parse_args(["--radiomics", "--survival", "--output_path", str(tmp_path / "out"), "--data_loc", str(tmp_path / "c.csv"),
                                         *loc, *FLAGS[flags]])
    parser = M.Parser(a.config)
    M.resolve_settings(a, parser)
    M.extract_radiomics_if_needed(parser, a)
    (n_tool, args_tool, kw_tool), (n_main, args_main, kw_main) = captured
    assert n_tool == n_main == 2 and args_tool == args_main == ()
    assert kw_tool == kw_main
    assert set(kw_main) == set(ALL_OFF)
    if (section, flags) in EXPECTED:
        assert kw_main == EXPECTED[(section, flags)]
    assert parser.config["Data"]["rad_loc"] == str(tmp_path / "out" / "radiomics_features.csv")


def test_the_tool_only_flags_go_before_the_config(tmp_path, captured):
    (tmp_path / "tree" / "t1").mkdir(parents=True)
    cfg = tiny_config(tmp_path, radiomics={"classes": ["gldm"]})
    radiomics.main(["--config", cfg, "--image_loc", str(tmp_path / "tree"), "--key_loc", "k.csv", "--out", str(tmp_path / "tool.csv"), "--classes", "all",
                    "--glszm"])
    (n, _, kw), = captured
    assert n == 1 and kw == dict(ALL_OFF, classes=tuple(radiomics.TEXTURE_CLASSES), glszm=True)


@pytest.mark.parametrize("data,radiomics_section,message", [
    (None, {"bin_width": "wide"}, "Radiomics.bin_width / max_bins 'wide' / None are not numbers"),
    ({"format": "analyze"}, None, "Data.format 'analyze' is none of auto, nifti, dicom"),
    ({"mask_roi": " "}, None, "Data.mask_roi ' ' is not a ROI name (a non-empty string)"),
    ({"mask_resample": "always"}, None, "Data.mask_resample 'always' is none of auto, geometry, never"),
], ids=["bin_width", "format", "mask_roi", "mask_resample"])
def test_the_tool_refuses_what_main_refuses(tmp_path, monkeypatch, data, radiomics_section, message):
    """The config values that only main.py used to refuse: the tool now ends with the same ConfigurationError."""
    from mmnn_sts_amd.exceptions.exceptions import ConfigurationError
    (tmp_path / "tree" / "t1").mkdir(parents=True)
    monkeypatch.setattr(radiomics, "extract_modalities", lambda *a, **k: pytest.fail("the extraction was reached"))
    cfg = tiny_config(tmp_path, radiomics=radiomics_section, data=data)
    with pytest.raises(ConfigurationError) as e:
        radiomics.main(["--config", cfg, "--image_loc", str(tmp_path / "tree"), "--key_loc", "k.csv", "--out", str(tmp_path / "tool.csv")])
    assert str(e.value) == message
