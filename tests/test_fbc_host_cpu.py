"""CPU: the host side of the background-conditioned IC-Light model (generation.iclight_model: fbc; utils/model_utils.py:97-179 init_iclight_bg) --
the 12-channel loader, hostlogic.check_fbc and the early refusals of run.py / invert.py, the config surface, the ramp and matte references and
the C ABI."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import fbc_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- loader
def test_full_size_fbc_pair_loads_strict_and_the_fc_call_is_unchanged(tmp_path):
    """A zero-filled full-size pair with the HF layout (UNet: 4 input channels, as published; offset files: the same keys with conv_in [320,12,3,3]
    for fbc, [320,8,3,3] for fc) through the loader init_iclight uses; one tensor of each file carries a marker so the merge is visible."""
    from safetensors.torch import save_file
    from test_checkpoint_layout_cpu import hf_unet_layout
    from tc_light_amd import model_utils, sd15
    hf = hf_unet_layout()
    base = {k: torch.zeros(s, dtype=torch.float16) for k, s in hf.items()}
    base["mid_block.resnets.0.conv1.bias"][7] = 1.5
    base["conv_in.weight"][3, 2, 1, 1] = 0.25
    pu = str(tmp_path / "unet.safetensors")
    save_file(base, pu)
    del base
    paths = {}
    for name, cin, mark in (("fc", 8, (3, 6, 1, 1)), ("fbc", 12, (3, 10, 1, 1))):
        off = {k: torch.zeros((320, cin, 3, 3) if k == "conv_in.weight" else s, dtype=torch.float16) for k, s in hf.items()}
        off["mid_block.resnets.0.conv1.bias"][7] = 0.5
        off["conv_in.weight"][mark] = -0.125
        off["conv_in.weight"][5, 4, 0, 2] = 0.5
        paths[name] = str(tmp_path / f"iclight_sd15_{name}.safetensors")
        save_file(off, paths[name])
        del off
    sd = model_utils.load_unet_state(pu, paths["fbc"], cond_channels=8)
    want = sd15.unet_param_shapes(in_channels=12)
    assert set(sd) == set(want) and all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    w = sd["conv_in.weight"]
    assert w.shape == (320, 12, 3, 3)
    assert float(sd["mid_block.resnets.0.conv1.bias"][7]) == 2.0                                    # W_sd15 + W_offset
    assert float(w[3, 2, 1, 1]) == 0.25 and float(w[3, 10, 1, 1]) == -0.125 and float(w[5, 4, 0, 2]) == 0.5
    assert float(w[:, 4:].abs().sum()) == 0.625 and float(w[:, :4].abs().sum()) == 0.25             # channels 4-11: zero + the offset
    del sd
    # the other model's offset file is refused, and the message names both shapes
    with pytest.raises(KeyError, match=r"(?s)\(320, 8, 3, 3\).*\(320, 12, 3, 3\)"):
        model_utils.load_unet_state(pu, paths["fc"], cond_channels=8)
    with pytest.raises(KeyError, match=r"(?s)\(320, 12, 3, 3\).*\(320, 8, 3, 3\)"):
        model_utils.load_unet_state(pu, paths["fbc"])
    with pytest.raises(ValueError, match="cond_channels"):
        model_utils.load_unet_state(pu, paths["fbc"], cond_channels=12)
    # the existing call: the same tensors with and without the new parameter spelled out
    a = model_utils.load_unet_state(pu, paths["fc"])
    assert a["conv_in.weight"].shape == (320, 8, 3, 3) and set(a) == set(sd15.unet_param_shapes())
    assert float(a["conv_in.weight"][3, 2, 1, 1]) == 0.25 and float(a["conv_in.weight"][3, 6, 1, 1]) == -0.125
    assert float(a["conv_in.weight"][:, 4:].abs().sum()) == 0.625 and float(a["mid_block.resnets.0.conv1.bias"][7]) == 2.0
    b = model_utils.load_unet_state(pu, paths["fc"], cond_channels=4)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_seeded_stand_ins_take_the_width(monkeypatch):
    from tc_light_amd import model_utils, sd15
    seen = {}

    def fake(shapes, seed, gain=1.0):                           # the full random dict is 860 M draws: only the request is of interest here
        seen["shape"], seen["seed"] = tuple(shapes["conv_in.weight"]), seed
        return {"conv_in.weight": torch.zeros(shapes["conv_in.weight"])}
    monkeypatch.setattr(sd15, "random_state_dict", fake)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert model_utils.load_unet_state(None, None, allow=True, cond_channels=8)["conv_in.weight"].shape == (320, 12, 3, 3)
        assert seen == dict(shape=(320, 12, 3, 3), seed=1)
        assert model_utils.load_unet_state(None, None, allow=True)["conv_in.weight"].shape == (320, 8, 3, 3)
        assert seen == dict(shape=(320, 8, 3, 3), seed=1)
    with pytest.raises(FileNotFoundError):
        model_utils.load_unet_state(None, None, cond_channels=8)


def test_a_narrow_conv_in_lora_goes_to_the_first_four_of_twelve():
    from tc_light_amd import lora as L
    g = torch.Generator().manual_seed(0)
    down, up = torch.randn(2, 4, 3, 3, generator=g), torch.randn(320, 2, 1, 1, generator=g)
    for cin in (8, 12):
        d, narrow = L._delta("conv_in.weight", torch.zeros(320, cin, 3, 3), down, up)
        assert narrow and tuple(d.shape) == (320, 4, 3, 3)
    with pytest.raises(ValueError):
        L._delta("conv_in.weight", torch.zeros(320, 16, 3, 3), down, up)


# ---------------------------------------------------------------------------------------------------------------- check_fbc
def test_check_fbc():
    from tc_light_amd import hostlogic as HL
    from tc_light_amd.generate import DEFAULTS
    assert (DEFAULTS["iclight_model"], DEFAULTS["bg_source"], DEFAULTS["fbc_matting"]) == ("fc", "upload", True)
    assert HL.check_fbc("fc", "upload") == ("fc", "upload") and HL.check_fbc(None, None) == ("fc", "upload")
    assert HL.check_fbc("FBC", "Left") == ("fbc", "left")
    for s in HL.BG_SOURCES:
        assert HL.check_fbc("fbc", s) == ("fbc", s)
    assert HL.BG_SOURCES == ("upload", "upload_flip", "left", "right", "top", "bottom", "grey")
    # fc: the other features are none of check_fbc's business
    assert HL.check_fbc("fc", "grey", "left", 1.5, True, True) == ("fc", "grey")
    for bad in ("fcb", "", 12, True):
        with pytest.raises(ValueError, match="iclight_model"):
            HL.check_fbc(bad, "upload")
    for bad in ("diagonal", "none", 3):
        with pytest.raises(ValueError, match="bg_source"):
            HL.check_fbc("fbc", bad)
    with pytest.raises(ValueError, match="(?s)fbc.*init_latent"):
        HL.check_fbc("fbc", "left", init_latent="left")
    with pytest.raises(ValueError, match="(?s)fbc.*highres_scale"):
        HL.check_fbc("fbc", "left", highres_scale=1.5)
    with pytest.raises(ValueError, match="(?s)fbc.*background_cond"):
        HL.check_fbc("fbc", "left", background_cond=True)
    with pytest.raises(ValueError, match="(?s)fbc.*inversion"):
        HL.check_fbc("fbc", "left", inversion=True)
    assert HL.cond_channels("fc") == 4 and HL.cond_channels("fbc") == 8
    # the uploaded background: one frame for all, or one per frame of the run
    assert HL.fbc_background_per_frame(1, 5) is False and HL.fbc_background_per_frame(5, 5) is True and HL.fbc_background_per_frame(1, 1) is False
    for n_bg, n in ((3, 2), (2, 5), (0, 4), (6, 5)):
        with pytest.raises(ValueError, match=f"(?s){n_bg} frames.*1 or exactly {n}"):
            HL.fbc_background_per_frame(n_bg, n, "upload_flip")
    assert {k: v[1:] for k, v in HL.BG_RAMPS.items()} == {k: v[1:] for k, v in R.RAMPS.items()}
    assert {k: "xxyy"[v[0]] for k, v in HL.BG_RAMPS.items()} == {k: v[0] for k, v in R.RAMPS.items()}


def _boom(monkeypatch):
    import invert
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.iclight_model / bg_source were checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(invert, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    return run, invert


def _cfg(tmp_path, keys):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}, {keys}}}
""")
    return str(cfg)


@pytest.mark.parametrize("keys,word", [("iclight_model: fbc, bg_source: left, init_latent: left", "(?s)fbc.*init_latent"),
                                       ("iclight_model: fbc, bg_source: left, init_latent: source", "(?s)fbc.*init_latent"),
                                       ("iclight_model: fbc, bg_source: grey, highres_scale: 1.5", "(?s)fbc.*highres_scale"),
                                       ("iclight_model: fbc, background_cond: true, background_image_path: bg.png", "(?s)fbc.*background_cond"),
                                       ("iclight_model: fcb", "iclight_model"), ("iclight_model: fbc, bg_source: diagonal", "bg_source"),
                                       ("bg_source: diagonal", "bg_source"),
                                       ("iclight_model: fbc, bg_source: upload", "background_image_path")])
def test_run_refuses_before_models(tmp_path, monkeypatch, keys, word):
    run, _ = _boom(monkeypatch)
    with pytest.raises(ValueError, match=word):
        run.main(["--config", _cfg(tmp_path, keys)])


@pytest.mark.parametrize("keys,word", [("iclight_model: fbc, bg_source: left", "(?s)fbc.*inversion"), ("iclight_model: fbc", "(?s)fbc.*inversion"),
                                       ("iclight_model: fcb", "iclight_model"), ("bg_source: diagonal", "bg_source")])
def test_invert_refuses_before_models(tmp_path, monkeypatch, keys, word):
    _, invert = _boom(monkeypatch)
    with pytest.raises(ValueError, match=word):
        invert.main(["--config", _cfg(tmp_path, keys)])


def test_cli_flags_are_refused_before_models_too(tmp_path, monkeypatch):
    run, _ = _boom(monkeypatch)
    cfg = _cfg(tmp_path, "init_latent: left")
    with pytest.raises(ValueError, match="(?s)fbc.*init_latent"):
        run.main(["--config", cfg, "--iclight_model", "fbc", "--bg_source", "left"])
    with pytest.raises(SystemExit):                             # argparse knows the names
        run.main(["--config", cfg, "--bg_source", "diagonal"])
    with pytest.raises(SystemExit):
        run.main(["--config", cfg, "--iclight_model", "fcb"])


def test_generator_refuses_too():
    """Whoever builds a Generator gets the same refusals, before its first kernel launch."""
    from types import SimpleNamespace
    from tc_light_amd.generate import Generator
    stub = SimpleNamespace(dev=torch.device("cpu"), tome=SimpleNamespace(args={}))
    for cfg, word in ((dict(iclight_model="fbc", bg_source="left", init_latent="left"), "(?s)fbc.*init_latent"),
                      (dict(iclight_model="fbc", bg_source="left", highres_scale=2.0), "(?s)fbc.*highres_scale"),
                      (dict(iclight_model="fbc", bg_source="left", background_cond=True), "(?s)fbc.*background_cond"),
                      (dict(iclight_model="fcb"), "iclight_model"), (dict(bg_source="diagonal"), "bg_source")):
        with pytest.raises(ValueError, match=word):
            Generator(stub, None, dict(cfg, max_tokens_per_pass=1))
    g = Generator(stub, None, dict(iclight_model="fbc", bg_source="grey", max_tokens_per_pass=1))
    assert g.fbc and g.cfg.bg_source == "grey" and g.cfg.fbc_matting is True
    assert not Generator(stub, None, dict(max_tokens_per_pass=1)).fbc
    # a UNet of the other width is refused by name
    stub8 = SimpleNamespace(dev=torch.device("cpu"), tome=SimpleNamespace(args={}), w={"conv_in": (None, None, 8)})
    with pytest.raises(ValueError, match="conv_in"):
        Generator(stub8, None, dict(iclight_model="fbc", bg_source="grey", max_tokens_per_pass=1))
    assert not Generator(stub8, None, dict(max_tokens_per_pass=1)).fbc


def test_example_config_and_cli_flags():
    from tc_light_amd.config_utils import load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_fbc.yaml")], print_config=False)
        assert c.generation.iclight_model == "fbc" and c.generation.bg_source == "left" and c.generation.fbc_matting is True
        assert c.models.iclight_offset.endswith("iclight_sd15_fbc.safetensors") and c.models.unet      # the other model paths are inherited
        assert isinstance(c.generation.prompt, dict) and all(isinstance(p, str) and p for p in c.generation.prompt.values())
        assert not c.generation.background_cond and c.generation.get("init_latent", "none") == "none"
        d = load_config(["--config", os.path.join("configs", "tclight_default.yaml")], print_config=False)
        assert not {"iclight_model", "bg_source", "fbc_matting"} & set(d.generation)               # the reference YAMLs stay as they are
        e = load_config(["--config", os.path.join("configs", "tclight_default.yaml"), "--iclight_model", "fbc", "--bg_source", "top"],
                        print_config=False)
        assert e.generation.iclight_model == "fbc" and e.generation.bg_source == "top"
    finally:
        os.chdir(cwd)


# ---------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_ramp_reference_is_numpy_linspace(n):
    for start, stop in ((224, 32), (32, 224), (64, 64), (255, 0)):
        want = np.linspace(start, stop, n).astype(np.uint8)
        assert R.linspace_u8(start, stop, n).dtype == np.uint8 and R.linspace_u8(start, stop, n).tolist() == want.tolist(), (start, stop, n)
    assert R.ramp_u8("left", 3, n).tolist() == [np.linspace(224, 32, n).astype(np.uint8).tolist()] * 3
    assert R.ramp_u8("right", 2, n).tolist() == [np.linspace(32, 224, n).astype(np.uint8).tolist()] * 2
    assert R.ramp_u8("top", n, 2).T.tolist() == [np.linspace(224, 32, n).astype(np.uint8).tolist()] * 2
    assert R.ramp_u8("bottom", n, 3).T.tolist() == [np.linspace(32, 224, n).astype(np.uint8).tolist()] * 3
    assert (R.ramp_u8("grey", n, 5) == 64).all() and R.ramp_u8("grey", n, 5).shape == (n, 5)


def test_matte_reference_is_the_recipe():
    """127 + (u - 127) a, truncated: a = 0 is the grey, a = 1 the pixel itself, a = 0.5 half way (toward 127, then truncated)."""
    us = [0, 126, 127, 128, 255]
    f = (np.array(us, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    assert ((np.float32(255.0) * f).astype(np.float32) == np.array(us, dtype=np.float32)).all()      # these five survive the round trip
    assert R.matte_q(f, 0.0).tolist() == [127] * 5
    assert R.matte_q(f, 1.0).tolist() == us
    assert R.matte_q(f, 0.5).tolist() == [63, 126, 127, 127, 191]                                  # 63.5, 126.5, 127, 127.5, 191 truncated
    grid = R.matte_q(f[:, None], np.array([0.0, 0.5, 1.0], dtype=np.float32)[None, :])
    assert grid.shape == (5, 3) and grid.dtype == np.int64 and grid.min() >= 0 and grid.max() <= 255
    assert R.matte_q(np.float32(2.0), 1.0) == 255 and R.matte_q(np.float32(-1.0), 1.0) == 0        # the clamp


def test_pack_reference_layout():
    g = torch.Generator().manual_seed(0)
    x, fg, bg = (torch.randn(5, 4, 3, 5, generator=g).half() for _ in range(3))
    out = R.pack12(x, fg, bg[:1], [4, 0, 4], 0)
    assert out.shape == (6, 3, 5, 12) and torch.equal(out[:3], out[3:])
    assert torch.equal(out[0, 1, 2], torch.cat([x[4, :, 1, 2], fg[4, :, 1, 2], bg[0, :, 1, 2]]))
    out = R.pack12(x, fg, bg, [3, 0], 1, sl=1, nwin=3)
    assert out.shape == (4, 3, 3, 12) and torch.equal(out[:2], out[2:])
    assert torch.equal(out[1, 2, 1], torch.cat([x[3, :, 1, 0], fg[3, :, 1, 0], bg[3, :, 1, 0]]))      # column 0, frame sl + 2, row 1


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH, parse_header
    if not os.path.exists(LIB_PATH):
        g.build()
    sig = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("tcl_pack_latents12_f16", 13), ("tcl_matte_grey_f32", 7), ("tcl_bg_ramp_f32", 7)):
        assert name in sig and len(sig[name][1]) == nargs and hasattr(dll, name), name
    assert len(sig["tcl_pack_latents_f16"][1]) == 11                # the 8-channel entry is untouched
