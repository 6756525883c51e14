"""CPU: the host side of the highres pass (generation.highres_scale / highres_denoise; IC-Light's process(), second half) -- the size rule, the
checks, run.py's early refusals, the config surface, the unchanged defaults of the Generator and the C ABI."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the size rule and the checks
def test_size_rule():
    from tc_light_amd import hostlogic as HL
    assert HL.highres_size(720, 1280, 1.5) == (1088, 1920)
    assert HL.highres_size(720, 960, 1.5) == (1088, 1408)              # 960 * 1.5 / 64 = 22.5 rounds half to even: 22 * 64, not 1472
    assert HL.highres_size(536, 960, 1.5) == (832, 1408)
    assert HL.highres_size(64, 64, 2.0) == (128, 128) and HL.highres_size(128, 192, 1.5) == (192, 256)
    assert HL.highres_size(720, 1280, 1.0) == (704, 1280)              # the rule itself always rounds; scale 1.0 never reaches it (off)
    assert all(isinstance(v, int) for v in HL.highres_size(720, 1280, 1.5))
    for h, w, s in ((16, 64, 1.0), (31, 640, 1.0), (64, 20, 1.5)):
        with pytest.raises(ValueError, match="below 64"):
            HL.highres_size(h, w, s)


def test_check_highres():
    from tc_light_amd import hostlogic as HL
    from tc_light_amd.generate import DEFAULTS
    assert (DEFAULTS["highres_scale"], DEFAULTS["highres_denoise"]) == (1.0, 0.5)
    assert HL.check_highres(1.0, 0.5) == (1.0, 0.5) and HL.check_highres(1, 1) == (1.0, 1.0) and HL.check_highres(3, 0.25, 25) == (3.0, 0.25)
    for bad in (0.99, 0, -1.5, 3.01, float("nan"), float("inf"), "1.5", None, True):
        with pytest.raises(ValueError, match="highres_scale"):
            HL.check_highres(bad, 0.5)
    for bad in (0, 0.0, -0.1, 1.01, float("nan"), "0.5", None, False):
        with pytest.raises(ValueError, match="highres_denoise"):
            HL.check_highres(1.5, bad)
    assert HL.img2img_schedule(1, 0.3)[2] == 0
    with pytest.raises(ValueError, match="no step"):
        HL.check_highres(1.5, 0.3, 1)
    assert HL.check_highres(1.0, 0.3, 1) == (1.0, 0.3)                  # off: the second schedule never runs
    with pytest.raises(ValueError, match="(?s)background_cond.*highres_scale"):
        HL.check_highres(1.5, 0.5, 25, background_cond=True)
    assert HL.check_highres(1.0, 0.5, 25, background_cond=True) == (1.0, 0.5)


# ---------------------------------------------------------------------------------------------------------------- run.py and the config surface
def _boom(monkeypatch):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.highres_scale / highres_denoise were checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    return run


def _cfg(tmp_path, keys, data="height: 64, width: 64"):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{{data}}}
generation: {{prompt: {{edit: "warm light"}}, {keys}}}
""")
    return str(cfg)


@pytest.mark.parametrize("keys,word", [("highres_scale: 0.5", "highres_scale"), ("highres_scale: 3.5", "highres_scale"),
                                       ("highres_scale: big", "highres_scale"), ("highres_scale: 1.5, highres_denoise: 0", "highres_denoise"),
                                       ("highres_denoise: 1.5", "highres_denoise"), ("highres_scale: 2, highres_denoise: -0.2", "highres_denoise"),
                                       ("highres_scale: 1.5, highres_denoise: 0.3, n_timesteps: 1", "no step"),
                                       ("highres_scale: 1.5, background_cond: true", "(?s)background_cond.*highres_scale")])
def test_run_refuses_before_models(tmp_path, monkeypatch, keys, word):
    run = _boom(monkeypatch)
    with pytest.raises(ValueError, match=word):
        run.main(["--config", _cfg(tmp_path, keys)])


def test_run_refuses_a_size_below_64_before_models(tmp_path, monkeypatch):
    run = _boom(monkeypatch)
    with pytest.raises(ValueError, match="below 64"):
        run.main(["--config", _cfg(tmp_path, "highres_scale: 1.2", data="height: 16, width: 64")])


def test_final_size_must_fit_the_vidtome_match(tmp_path, monkeypatch):
    """(chunk_size - 1) frames' level-0 tokens are the sources of one VidToMe match; the match kernels take 64 K of them."""
    from tc_light_amd import hostlogic as HL
    assert HL.TOME_MAX_SRC_TOKENS == 65536
    HL.check_highres_tokens(832, 1408, 4)                               # 3 * 104 * 176 = 54 912: the example config
    HL.check_highres_tokens(1088, 1920, 2)                              # 32 640
    HL.check_highres_tokens(1088, 1920, 1)
    with pytest.raises(ValueError, match="(?s)highres_scale.*chunk_size"):
        HL.check_highres_tokens(1088, 1920, 4)                          # 97 920
    run = _boom(monkeypatch)
    with pytest.raises(ValueError, match="(?s)highres_scale.*chunk_size"):
        run.main(["--config", _cfg(tmp_path, "highres_scale: 1.5", data="height: 720, width: 1280")])


def test_run_refuses_cli_values_before_models(tmp_path, monkeypatch):
    run = _boom(monkeypatch)
    cfg = _cfg(tmp_path, "n_timesteps: 2")
    for s in ("0.5", "3.5", "nan"):
        with pytest.raises(ValueError, match="highres_scale"):
            run.main(["--config", cfg, "--highres_scale", s])
    for s in ("0", "-0.1", "1.5"):
        with pytest.raises(ValueError, match="highres_denoise"):
            run.main(["--config", cfg, "--highres_scale", "1.5", "--highres_denoise", s])


def test_example_config_and_cli_flags():
    from tc_light_amd.config_utils import load_config
    from tc_light_amd import hostlogic as HL
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_highres.yaml")], print_config=False)
        assert HL.check_highres(c.generation.highres_scale, c.generation.highres_denoise, c.generation.n_timesteps) == (1.5, 0.5)
        assert HL.highres_size(c.data.height, c.data.width, c.generation.highres_scale) == (832, 1408)
        assert isinstance(c.generation.prompt, dict) and all(isinstance(p, str) and p for p in c.generation.prompt.values())
        d = load_config(["--config", os.path.join("configs", "tclight_default.yaml")], print_config=False)
        assert "highres_scale" not in d.generation and "highres_denoise" not in d.generation      # the reference YAMLs stay as they are
        e = load_config(["--config", os.path.join("configs", "tclight_default.yaml"), "--highres_scale", "2", "--highres_denoise", "0.4"],
                        print_config=False)
        assert e.generation.highres_scale == 2.0 and e.generation.highres_denoise == 0.4
    finally:
        os.chdir(cwd)


# ---------------------------------------------------------------------------------------------------------------- the Generator's defaults
def _stub_unet():
    return SimpleNamespace(dev=torch.device("cpu"), tome=SimpleNamespace(args={}))


def test_defaults_leave_schedule_and_rng_as_they_were(monkeypatch):
    """highres_scale 1.0 (the default, or spelled out with any highres_denoise): the same schedule, no second one, and prepare_data draws from the
    RNG exactly what it drew before -- the state of the generator after it equals that after the one randn it stands for."""
    import tc_light_amd.generate as G
    monkeypatch.setattr(G, "lib", lambda: None)
    for mode, shape in (("same", (1, 4, 8, 8)), ("vanilla", (3, 4, 8, 8))):
        base = dict(n_timesteps=5, seed=21, noise_mode=mode, max_tokens_per_pass=1 << 20)
        ga, gb = G.Generator(_stub_unet(), None, base), G.Generator(_stub_unet(), None, dict(base, highres_scale=1.0, highres_denoise=0.25))
        assert not ga.highres and not gb.highres and ga.schedule_highres is None and gb.schedule_highres is None
        assert ga.schedule == gb.schedule == (5, 0, 5) and not ga.img2img
        rng = torch.Generator(device="cpu").manual_seed(21)
        z = torch.randn(*shape, generator=rng, dtype=torch.float32)
        for g in (ga, gb):
            g.prepare_data(torch.zeros(3, 3, 64, 64))
            assert torch.equal(g.rng_dev.get_state(), rng.get_state())
            assert torch.equal(g.init_noise, (z * g.scheduler.init_noise_sigma).to(torch.float16).expand(3, -1, -1, -1))
    on = G.Generator(_stub_unet(), None, dict(base, highres_scale=1.5, highres_denoise=0.25))
    assert on.highres and on.schedule == (5, 0, 5) and on.schedule_highres == (20, 15, 5)
    for bad in (dict(highres_scale=0.5), dict(highres_scale=1.5, highres_denoise=0), dict(highres_scale=2, highres_denoise=0.3, n_timesteps=1)):
        with pytest.raises(ValueError, match="highres"):
            G.Generator(_stub_unet(), None, dict(base, **bad))


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH, parse_header
    if not os.path.exists(LIB_PATH):
        g.build()
    sig = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("tcl_frames_to_u8", 6), ("tcl_u8_to_frames_f32", 7), ("tcl_resize_lanczos_table_ints", 2), ("tcl_resize_lanczos_table", 3),
                        ("tcl_resize_lanczos_u8", 10)):
        assert name in sig and len(sig[name][1]) == nargs and hasattr(dll, name), name
    assert sig["tcl_resize_lanczos_table_ints"][0] is ctypes.c_size_t and sig["tcl_u8_to_frames_f32"][1][5] is ctypes.c_float
