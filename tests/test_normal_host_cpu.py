"""CPU: the host side of generation.normal (IC-Light's "Compute Normal" on the fbc model) -- hostlogic.check_normal, the default, the config surface
(YAML key, --normal, the example), run.py's refusal before any model is loaded, and the C ABI of the two new entries."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_normal():
    from tc_light_amd import hostlogic as HL
    from tc_light_amd.generate import DEFAULTS
    assert DEFAULTS["normal"] is False
    assert HL.check_normal(True, "fbc", True, True) == ("left", "right", "bottom", "top")          # the demo's order
    assert HL.check_normal(True, "FBC", False, False) == ("left", "right", "bottom", "top")
    assert HL.NORMAL_SIDES == ("left", "right", "bottom", "top") and all(s in HL.BG_RAMPS for s in HL.NORMAL_SIDES)
    assert HL.NORMAL_MATTE_SIGMA == 16.0
    for model in ("fc", "fbc", None):                                   # off: nothing else is looked at
        assert HL.check_normal(False, model, True, True) == () and HL.check_normal(None, model) == ()
    for model in ("fc", None):
        with pytest.raises(ValueError, match="(?s)generation.normal.*generation.iclight_model"):
            HL.check_normal(True, model, True, True)
    for bad in ("yes", 1, 0.5):
        with pytest.raises(ValueError, match="generation.normal"):
            HL.check_normal(bad, "fbc", True, True)
    with pytest.raises(ValueError, match="(?s)generation.normal.*fbc_matting"):
        HL.check_normal(True, "fbc", "no", True)
    with pytest.raises(ValueError, match="(?s)generation.normal.*apply_opt"):
        HL.check_normal(True, "fbc", True, "no")


def _cfg(tmp_path, keys):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}, {keys}}}
""")
    return str(cfg)


def _boom(monkeypatch):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.normal was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    return run


def test_run_refuses_normal_under_fc_before_models(tmp_path, monkeypatch):
    run = _boom(monkeypatch)
    with pytest.raises(ValueError, match="(?s)generation.normal.*generation.iclight_model"):
        run.main(["--config", _cfg(tmp_path, "alpha_t: 0.0"), "--normal", "--iclight_model", "fc"])
    with pytest.raises(ValueError, match="(?s)generation.normal.*generation.iclight_model"):
        run.main(["--config", _cfg(tmp_path, "normal: true")])                                      # the YAML key, the default model
    with pytest.raises(ValueError, match="generation.normal"):
        run.main(["--config", _cfg(tmp_path, "normal: 3, iclight_model: fbc, bg_source: left")])
    # what fbc itself refuses stays refused under normal
    with pytest.raises(ValueError, match="(?s)fbc.*highres_scale"):
        run.main(["--config", _cfg(tmp_path, "normal: true, iclight_model: fbc, highres_scale: 1.5")])
    # (under normal bg_source is not consulted: tests/test_gpu_normal.py runs `bg_source: upload` without a background_image_path)
    with pytest.raises(ValueError, match="background_image_path"):                                  # without normal it still is asked for
        run.main(["--config", _cfg(tmp_path, "iclight_model: fbc, bg_source: upload")])


def test_generator_refuses_too():
    from types import SimpleNamespace
    from tc_light_amd.generate import Generator
    stub = SimpleNamespace(dev=torch.device("cpu"), tome=SimpleNamespace(args={}))
    with pytest.raises(ValueError, match="(?s)generation.normal.*generation.iclight_model"):
        Generator(stub, None, dict(normal=True, max_tokens_per_pass=1))
    g = Generator(stub, None, dict(normal=True, iclight_model="fbc", bg_source="grey", max_tokens_per_pass=1))
    assert g.normal_sides == ("left", "right", "bottom", "top")
    g = Generator(stub, None, dict(iclight_model="fbc", bg_source="grey", max_tokens_per_pass=1))
    assert g.normal_sides == ()
    with pytest.raises(ValueError, match="generation.normal"):          # normals() of a Generator built without the key
        g.normals(None, None, None)


def test_example_config_and_cli_flag():
    from tc_light_amd.config_utils import load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_normal.yaml")], print_config=False)
        assert c.generation.normal is True and c.generation.iclight_model == "fbc" and c.generation.fbc_matting is True
        assert c.models.iclight_offset.endswith("iclight_sd15_fbc.safetensors") and c.models.unet
        assert isinstance(c.generation.prompt, dict) and all(isinstance(p, str) and p for p in c.generation.prompt.values())
        d = load_config(["--config", os.path.join("configs", "tclight_default.yaml")], print_config=False)
        assert "normal" not in d.generation                             # the reference YAMLs stay as they are
        e = load_config(["--config", os.path.join("configs", "tclight_default.yaml"), "--normal", "--iclight_model", "fbc"], print_config=False)
        assert e.generation.normal is True and e.generation.iclight_model == "fbc"
    finally:
        os.chdir(cwd)


def test_save_video_stem(tmp_path):
    """run.py writes the normal video through save_video under another stem; the default stem is untouched."""
    from tc_light_amd.dataparser import save_video
    fr = torch.rand(2, 3, 16, 16)
    a = save_video(fr, str(tmp_path), gif=False, stem="normal")
    b = save_video(fr, str(tmp_path), gif=False, post_fix="_gt")
    assert os.path.splitext(os.path.basename(a))[0] == "normal" and os.path.splitext(os.path.basename(b))[0] == "output_gt"
    assert os.path.exists(a) and os.path.exists(b)


def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH, parse_header
    if not os.path.exists(LIB_PATH):
        g.build()
    sig = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("tcl_matte_grey_sigma_f32", 8), ("tcl_fbc_normal", 12)):
        assert name in sig and len(sig[name][1]) == nargs and hasattr(dll, name), name
    assert sig["tcl_matte_grey_sigma_f32"][1][6] is ctypes.c_float
    assert len(sig["tcl_matte_grey_f32"][1]) == 7                       # the existing entry and its signature stay
