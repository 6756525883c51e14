"""CPU: the host side of the animated light (generation.light_path; --light_sweep) -- hostlogic.check_light_path / light_angles / light_dirs against
the restatements of tests/sweep_refs.py, every refused combination by both key names before a model is loaded (run.py and Generator), the default
left alone, the flag, the example YAML and the C ABI."""
import ctypes
import math
import os
from types import SimpleNamespace

import pytest
import torch

import sweep_refs as R
from tc_light_amd import hostlogic as HL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- keyframes
def test_keyframe_validation():
    assert HL.check_light_path(None) is None
    assert HL.check_light_path([[0, 30]]) == [[0.0, 30.0]]                                # a single keyframe: a constant direction
    assert HL.check_light_path([(0, -45), (0.5, 90.5), (1, 750)]) == [[0.0, -45.0], [0.5, 90.5], [1.0, 750.0]]
    assert HL.check_light_path([[0, 0], [0.5, 90], [0.5, 180], [1, 180]])[2] == [0.5, 180.0]      # non-decreasing: a jump is allowed
    out = HL.check_light_path([[0, 0], [1, 180]])
    assert all(type(v) is float for kf in out for v in kf) and HL.check_light_path(out) == out
    for bad in ([], (), "left", 90, [[0.5, 0], [1, 90]], [[0, 0], [0.9, 90]], [[0, 0], [0.7, 10], [0.3, 20], [1, 30]], [[0, NAN]],
                [[0, 0], [1, INF]], [[0, 0], [NAN, 5], [1, 10]], [[0, 0, 0]], [[0]], [0, 90], [[0, "90"]], [[0, True]], [[1, 90]],
                [[0, 0], [1, 90], [1.5, 100]], [[-0.5, 0], [1, 90]]):
        with pytest.raises(ValueError, match="light_path"):
            HL.check_light_path(bad)


def test_interpolation_values():
    sweep = HL.check_light_path([[0, 0], [1, 180]])
    assert HL.light_positions(3) == [0.0, 0.5, 1.0] and HL.light_positions(1) == [0.0] and HL.light_positions(5, 3, 5) == [0.75, 1.0]
    assert HL.light_angles(sweep, HL.light_positions(3)) == [0.0, 90.0, 180.0]
    assert HL.light_angles(sweep, HL.light_positions(1)) == [0.0]                        # N = 1: the first keyframe
    assert HL.light_angles(sweep, HL.light_positions(5)) == [0.0, 45.0, 90.0, 135.0, 180.0]
    turns = HL.check_light_path([[0, -90], [1, 810]])                                    # two and a half turns, no shortest arc
    assert HL.light_angles(turns, HL.light_positions(6)) == [-90.0, 90.0, 270.0, 450.0, 630.0, 810.0]
    assert HL.light_angles([[0.0, 350.0], [1.0, 10.0]], [0.5]) == [180.0]                # through 180, not through 0
    three = HL.check_light_path([[0, 0], [0.25, 100], [1, 40]])
    assert HL.light_angles(three, [0.0, 0.125, 0.25, 0.625, 1.0]) == [0.0, 50.0, 100.0, 70.0, 40.0]
    jump = HL.check_light_path([[0, 0], [0.5, 90], [0.5, 180], [1, 180]])
    assert HL.light_angles(jump, [0.25, 0.5, 0.75]) == [45.0, 180.0, 180.0]
    assert HL.light_angles([[0.0, 33.0]], HL.light_positions(4)) == [33.0] * 4
    for path, n in ((sweep, 7), (turns, 11), (three, 9), (jump, 6), ([[0.0, 33.0]], 3)):  # the restatement agrees, bit for bit
        assert HL.light_angles(path, HL.light_positions(n)) == R.angles(path, R.positions(n)) and HL.light_positions(n) == R.positions(n)
    # a rank of a sharded run takes the global positions of its own frames
    whole = HL.light_angles(sweep, HL.light_positions(5))
    assert HL.light_angles(sweep, HL.light_positions(5, 0, 3)) + HL.light_angles(sweep, HL.light_positions(5, 3, 5)) == whole


def test_exact_directions():
    assert HL.light_dirs([-90.0, 0.0, 450.0, 720.0]) == [(0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (1.0, 0.0)]
    assert HL.light_dirs([90.0, 180.0, 270.0, 360.0, -180.0, -360.0, -0.0]) == [(0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0),
                                                                               (1.0, 0.0), (1.0, 0.0)]
    assert all(math.copysign(1.0, v) == 1.0 for d in HL.light_dirs([0.0, 90.0, 180.0, 270.0]) for v in d if v == 0.0)      # no -0.0
    assert [HL.light_reduce(a) for a in (-45.0, 750.0, 359.999, -1e-20, -0.0, 360.0)] == [315.0, 30.0, 359.999, 0.0, 0.0, 0.0]
    assert math.copysign(1.0, HL.light_reduce(-0.0)) == 1.0
    assert [HL.light_axis_side(r) for r in (0.0, 90.0, 180.0, 270.0, 30.0, 89.99999999999999, 315.0)] == ["left", "top", "right", "bottom", None, None,
                                                                                                         None]
    (c, s), = HL.light_dirs([37.5])
    assert (c, s) == (math.cos(math.radians(37.5)), math.sin(math.radians(37.5)))
    assert HL.light_dirs([-45.0]) == [(math.cos(math.radians(315.0)), math.sin(math.radians(315.0)))]
    assert HL.light_dirs(list(R.ANGLES) + [0.0, 90.0, 180.0, 270.0]) == R.dirs(list(R.ANGLES) + [0.0, 90.0, 180.0, 270.0])
    assert HL.LIGHT_LEVELS == {"fc": (255, 0), "fbc": (224, 32)}
    assert {HL.BG_RAMPS[s][1:] for s in ("left", "top")} == {(224, 32)} and {HL.BG_RAMPS[s][1:] for s in ("right", "bottom")} == {(32, 224)}


# ---------------------------------------------------------------------------------------------------------------- combinations
PATH = [[0, 0], [1, 180]]
REFUSED = [(dict(init_latent="left"), "(?s)light_path.*init_latent"), (dict(init_latent="source"), "(?s)light_path.*init_latent"),
           (dict(normal=True, iclight_model="fbc"), "(?s)light_path.*normal"), (dict(normal=True), "(?s)light_path.*normal"),
           (dict(iclight_model="fbc", bg_source="left"), "(?s)light_path.*bg_source"),
           (dict(iclight_model="fbc", bg_source="grey"), "(?s)light_path.*bg_source"),
           (dict(iclight_model="fbc", bg_source="upload_flip"), "(?s)light_path.*bg_source")]


@pytest.mark.parametrize("keys,word", REFUSED)
def test_check_light_path_refuses_combinations(keys, word):
    with pytest.raises(ValueError, match=word):
        HL.check_light_path(PATH, **keys)
    assert HL.check_light_path(None, **keys) is None                                     # off: nothing of it is consulted


def test_allowed_combinations_and_the_default():
    assert HL.check_light_path(PATH, "none", False, "fc", "upload", 0.9, 25) == [[0.0, 0.0], [1.0, 180.0]]
    assert HL.check_light_path(PATH, None, None, None, None) == [[0.0, 0.0], [1.0, 180.0]]
    assert HL.check_light_path(PATH, iclight_model="fbc", bg_source="upload") and HL.check_light_path(PATH, iclight_model="fbc", bg_source=None)
    assert HL.check_light_path(PATH, iclight_model="fc", bg_source="left")                # fc: bg_source is none of its business
    with pytest.raises(ValueError, match="(?s)light_path.*init_strength"):               # fc: an img2img start, refused as check_init refuses it
        HL.check_light_path(PATH, init_strength=0.3, n_timesteps=1)
    assert HL.check_light_path(PATH, iclight_model="fbc", init_strength=0.3, n_timesteps=1)      # fbc: the plain schedule runs
    # light_path: null leaves the other checks' answers where they were
    assert HL.check_init("left", 0.5, 25) == ("left", 0.5) and HL.check_init(None, 1) == ("none", 1.0)
    assert HL.check_fbc("FBC", "Left") == ("fbc", "left") and HL.check_fbc(None, None) == ("fc", "upload")
    assert HL.check_normal(True, "fbc") == HL.NORMAL_SIDES and HL.check_normal(False) == ()


def _stub():
    return SimpleNamespace(dev=torch.device("cpu"), tome=SimpleNamespace(args={}))


def test_generator_refuses_too_and_takes_the_schedule_of_init_latent():
    from tc_light_amd.generate import DEFAULTS, Generator
    assert DEFAULTS["light_path"] is None
    for keys, word in REFUSED:
        with pytest.raises(ValueError, match=word):
            Generator(_stub(), None, dict(keys, light_path=PATH, max_tokens_per_pass=1))
        if not keys.get("normal") or keys.get("iclight_model") == "fbc":                  # without the path the same keys build as before
            Generator(_stub(), None, dict(keys, max_tokens_per_pass=1))
    with pytest.raises(ValueError, match="light_path"):
        Generator(_stub(), None, dict(light_path=[[0, 0], [0.5, 90]], max_tokens_per_pass=1))
    off = Generator(_stub(), None, dict(max_tokens_per_pass=1))
    assert off.cfg.light_path is None and not off.light and not off.img2img and off.schedule == (25, 0, 25)
    g = Generator(_stub(), None, dict(light_path=PATH, init_strength=0.5, n_timesteps=2, max_tokens_per_pass=1))
    left = Generator(_stub(), None, dict(init_latent="left", init_strength=0.5, n_timesteps=2, max_tokens_per_pass=1))
    assert g.light and g.img2img and g.cfg.init_latent == "none" and g.schedule == left.schedule == (4, 2, 2)
    hr = Generator(_stub(), None, dict(light_path=PATH, highres_scale=1.5, max_tokens_per_pass=1))       # the highres pass stays allowed under fc
    assert hr.highres and hr.light
    b = Generator(_stub(), None, dict(light_path=PATH, iclight_model="fbc", n_timesteps=2, init_strength=0.5, max_tokens_per_pass=1))
    assert b.light and b.fbc and not b.img2img and b.schedule == (2, 0, 2) and b.cfg.bg_source == "upload"


# ---------------------------------------------------------------------------------------------------------------- run.py, before any model
def _boom(monkeypatch):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.light_path was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    return run


def _cfg(tmp_path, keys):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}, {keys}}}
""")
    return str(cfg)


@pytest.mark.parametrize("keys,word", [("light_path: [[0, 0], [1, 180]], init_latent: left", "(?s)light_path.*init_latent"),
                                       ("light_path: [[0, 0], [1, 180]], iclight_model: fbc, normal: true", "(?s)light_path.*normal"),
                                       ("light_path: [[0, 0], [1, 180]], normal: true", "(?s)light_path.*normal"),
                                       ("light_path: [[0, 0], [1, 180]], iclight_model: fbc, bg_source: right", "(?s)light_path.*bg_source"),
                                       ("light_path: [[0, 0], [1, 180]], iclight_model: fbc, bg_source: upload_flip, background_image_path: b.png",
                                        "(?s)light_path.*bg_source"),
                                       ("light_path: []", "light_path"), ("light_path: [[0, 0], [0.5, 90]]", "light_path"),
                                       ("light_path: [[0.2, 0], [1, 90]]", "light_path"), ("light_path: [[0, 0], [0.6, 5], [0.4, 9], [1, 90]]", "light_path"),
                                       ("light_path: [[0, .nan]]", "light_path"), ("light_path: left", "light_path")])
def test_run_refuses_before_models(tmp_path, monkeypatch, keys, word):
    run = _boom(monkeypatch)
    with pytest.raises(ValueError, match=word):
        run.main(["--config", _cfg(tmp_path, keys)])


def test_cli_flag_is_refused_before_models_too(tmp_path, monkeypatch):
    run = _boom(monkeypatch)
    with pytest.raises(ValueError, match="(?s)light_path.*init_latent"):
        run.main(["--config", _cfg(tmp_path, "init_latent: top"), "--light_sweep", "0", "180"])
    with pytest.raises(ValueError, match="(?s)light_path.*init_latent"):
        run.main(["--config", _cfg(tmp_path, "n_timesteps: 2"), "--light_sweep", "0", "180", "--light", "left"])
    with pytest.raises(ValueError, match="(?s)light_path.*bg_source"):
        run.main(["--config", _cfg(tmp_path, "n_timesteps: 2"), "--light_sweep", "0", "180", "--iclight_model", "fbc", "--bg_source", "left"])
    with pytest.raises(SystemExit):                                                      # two numbers
        run.main(["--config", _cfg(tmp_path, "n_timesteps: 2"), "--light_sweep", "0"])
    with pytest.raises(SystemExit):
        run.main(["--config", _cfg(tmp_path, "n_timesteps: 2"), "--light_sweep", "left", "right"])


def test_fbc_path_needs_no_background_file(tmp_path, monkeypatch):
    """Under fbc the ramps are the backgrounds: bg_source stays at its default `upload`, and run.py must not ask for background_image_path.  It gets
    as far as the model loader (made to fail here)."""
    run = _boom(monkeypatch)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)                       # run.py picks its device just before the loader
    with pytest.raises(AssertionError, match="a model was loaded"):
        run.main(["--config", _cfg(tmp_path, "light_path: [[0, 0], [1, 180]], iclight_model: fbc")])
    with pytest.raises(ValueError, match="background_image_path"):                        # without the path: as before
        run.main(["--config", _cfg(tmp_path, "iclight_model: fbc")])


# ---------------------------------------------------------------------------------------------------------------- config surface
def test_example_config_and_cli_flag():
    from tc_light_amd.config_utils import load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_light_sweep.yaml")], print_config=False)
        assert HL.check_light_path(c.generation.light_path, c.generation.get("init_latent"), c.generation.get("normal"),
                                   c.generation.get("iclight_model"), c.generation.get("bg_source")) == [[0.0, 0.0], [1.0, 180.0]]
        assert c.generation.init_strength == 0.9 and c.generation.get("init_latent", "none") == "none" and c.models.unet
        assert isinstance(c.generation.prompt, dict) and all(isinstance(p, str) and p for p in c.generation.prompt.values())
        d = load_config(["--config", os.path.join("configs", "tclight_default.yaml")], print_config=False)
        assert "light_path" not in d.generation                                           # the reference YAMLs stay as they are
        e = load_config(["--config", os.path.join("configs", "tclight_default.yaml"), "--light_sweep", "-45", "405.5"], print_config=False)
        assert e.generation.light_path == [[0.0, -45.0], [1.0, 405.5]] and HL.check_light_path(e.generation.light_path) == e.generation.light_path
        f = load_config(["--config", os.path.join("configs", "examples", "tclight_light_sweep.yaml"), "--light_sweep", "90", "90"],
                        print_config=False)
        assert f.generation.light_path == [[0.0, 90.0], [1.0, 90.0]]                     # the flag wins over the YAML
    finally:
        os.chdir(cwd)


def test_invert_ignores_the_key(tmp_path, monkeypatch):
    """invert.py reads nothing of generation.light_path: a malformed one does not stop it before the model loader (made to fail here)."""
    import invert
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("reached the model loader")
    monkeypatch.setattr(invert, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)
    with pytest.raises(AssertionError, match="reached the model loader"):
        invert.main(["--config", _cfg(tmp_path, "light_path: [[0.5, 0]]")])


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_symbol():
    from tc_light_amd.lib import LIB_PATH, parse_header
    sig = parse_header()
    assert sig["tcl_light_ramp_angle_f32"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                            ctypes.c_int, ctypes.c_void_p])
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(ctypes.CDLL(LIB_PATH), "tcl_light_ramp_angle_f32")
