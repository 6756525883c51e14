"""CPU: the host side of the light-direction / strength start (generation.init_latent, init_strength; IC-Light's "Lighting Preference") -- the
img2img schedule table, the scheduler's begin index against the oracle scheduler, run.py's early refusals, the config surface and the C ABI."""
import ctypes
import math
import os

import numpy as np
import pytest

import light_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("n", [1, 2, 3, 20, 25])
@pytest.mark.parametrize("s", [0.1, 0.3, 0.5, 0.6, 0.9, 0.99, 1.0])
def test_schedule_table(n, s):
    from tc_light_amd import hostlogic as HL
    got = HL.img2img_schedule(n, s)
    assert got == R.schedule(n, s) and all(isinstance(v, int) for v in got)
    n_sched, begin, run = got
    assert 0 <= begin <= n_sched and begin + run == n_sched and abs(run - n) <= 1
    if s == 1.0:
        assert got == (n, 0, n)


def test_schedule_spot_values():
    from tc_light_amd import hostlogic as HL
    assert HL.img2img_schedule(25, 0.9) == (28, 3, 25)
    assert HL.img2img_schedule(20, 0.9) == (22, 3, 19)          # one step short of n: the demo's behaviour, kept and reported
    assert HL.img2img_schedule(3, 0.6) == (5, 2, 3)


def test_check_init():
    from tc_light_amd import hostlogic as HL
    from tc_light_amd.generate import DEFAULTS
    assert (DEFAULTS["init_latent"], DEFAULTS["init_strength"]) == ("none", 0.9)
    assert HL.check_init("none", 0.9) == ("none", 0.9) and HL.check_init(None, 1) == ("none", 1.0) and HL.check_init("Left", 0.5, 25) == ("left", 0.5)
    for name in ("left", "right", "top", "bottom", "source"):
        assert HL.check_init(name, 1.0, 1) == (name, 1.0)
    for bad in ("diagonal", "", "ambient", 3):
        with pytest.raises(ValueError, match="init_latent"):
            HL.check_init(bad, 0.9)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="init_strength"):
            HL.check_init("left", bad)
    assert R.schedule(1, 0.3)[2] == 0                           # nothing left to execute: refused, as diffusers' img2img pipeline refuses it
    with pytest.raises(ValueError, match="no step"):
        HL.check_init("left", 0.3, 1)
    assert HL.check_init("none", 0.3, 1) == ("none", 0.3)       # not an img2img start: the plain schedule runs


# ---------------------------------------------------------------------------------------------------------------- scheduler
def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("n,begin", [(28, 3), (22, 3), (5, 2), (5, 4), (10, 9), (3, 0)])
def test_scheduler_begin_index_vs_oracle(n, begin):
    from oracle.scheduler import Scheduler as OSch
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    sch, osch = DPMSolverSDEScheduler(), OSch(n)
    sch.set_timesteps(n, begin)
    assert sch.timesteps.tolist() == osch.timesteps[begin:].tolist() and len(sch.timesteps) == n - begin
    # the sigma table stays whole, steps index it absolutely (the two tables are built from numpy / torch f32 betas: equal to an f32 ulp or two)
    assert sch.sigmas.shape == (n + 1,) and np.allclose(sch.sigmas, osch.sigmas.numpy(), rtol=4 * 2.0 ** -24, atol=0)
    sigma = float(sch.sigmas[begin])
    alpha, sigma_t = sch.add_noise_coefficients()
    assert alpha == 1.0 / math.sqrt(sigma * sigma + 1.0) and sigma_t == sigma * alpha
    # the first executed step: absolute index `begin`, first order (empty multistep history), whatever came before it in the table
    i, second = sch.next_step()
    assert (i, second) == (begin, False)
    co = sch.coefficients(i, second)
    assert co[4] == 0.0 and co[0] == sigma_t and co[1] == alpha
    # walking the host state as step() does: second order from the second executed step on, first order again on the absolute last index
    orders = []
    for _ in range(n - begin):
        i, second = sch.next_step()
        orders.append((i, second))
        sch._i += 1
        sch._lower = min(sch._lower + 1, sch.order)
    assert orders == [(begin + k, 0 < k and begin + k < n - 1) for k in range(n - begin)]
    assert sch.coefficients(n - 1, False)[2] == 0.0 and sch.coefficients(n - 1, False)[5] == 0.0      # last: sigma_next = 0, no noise term
    for bad in (-1, n, n + 3):
        with pytest.raises(ValueError):
            sch.set_timesteps(n, bad)


@pytest.mark.parametrize("n", [1, 3, 25])
def test_scheduler_begin_zero_is_the_plain_call(n):
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    a, b = DPMSolverSDEScheduler(), DPMSolverSDEScheduler()
    a.set_timesteps(n)
    b.set_timesteps(n, 0)
    assert sorted(vars(a)) == sorted(vars(b))
    for k in vars(a):
        assert _same(getattr(a, k), getattr(b, k)), k
    assert len(a.timesteps) == n and a.next_step() == (0, False) and DPMSolverSDEScheduler.order == 2


# ---------------------------------------------------------------------------------------------------------------- run.py and the config surface
def _boom(monkeypatch):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.init_latent / init_strength were checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    return run


@pytest.mark.parametrize("keys,word", [("init_latent: diagonal", "init_latent"), ("init_latent: front, init_strength: 0.5", "init_latent"),
                                       ("init_latent: left, init_strength: 0", "init_strength"), ("init_latent: left, init_strength: -0.1", "init_strength"),
                                       ("init_latent: source, init_strength: 1.5", "init_strength"), ("init_strength: 1.5", "init_strength"),
                                       ("init_latent: top, init_strength: 0.3, n_timesteps: 1", "no step")])
def test_run_refuses_before_models(tmp_path, monkeypatch, keys, word):
    run = _boom(monkeypatch)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}, {keys}}}
""")
    with pytest.raises(ValueError, match=word):
        run.main(["--config", str(cfg)])


def test_run_refuses_cli_strength_before_models(tmp_path, monkeypatch):
    run = _boom(monkeypatch)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}}}
""")
    for s in ("0", "-0.1", "1.5"):
        with pytest.raises(ValueError, match="init_strength"):
            run.main(["--config", str(cfg), "--light", "left", "--strength", s])
    with pytest.raises(SystemExit):                             # argparse knows the sides
        run.main(["--config", str(cfg), "--light", "diagonal"])


def test_example_config_and_cli_flags():
    from tc_light_amd.config_utils import load_config
    from tc_light_amd.generate import DEFAULTS
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_light_left.yaml")], print_config=False)
        assert c.generation.init_latent == "left" and 0 < c.generation.init_strength <= 1 and c.generation.n_timesteps == 25
        assert isinstance(c.generation.prompt, dict) and all(isinstance(p, str) and p for p in c.generation.prompt.values())
        assert "latents_path" in c.generation                   # the default YAML always sets it: not an error with init_latent
        d = load_config(["--config", os.path.join("configs", "tclight_default.yaml")], print_config=False)
        assert "init_latent" not in d.generation and "init_strength" not in d.generation      # the six reference YAMLs stay as they are
        e = load_config(["--config", os.path.join("configs", "tclight_default.yaml"), "--light", "left", "--strength", "0.8"], print_config=False)
        assert e.generation.init_latent == "left" and e.generation.init_strength == 0.8
        f = load_config(["--config", os.path.join("configs", "examples", "tclight_light_left.yaml"), "--light", "source"], print_config=False)
        assert f.generation.init_latent == "source" and f.generation.init_strength == c.generation.init_strength
    finally:
        os.chdir(cwd)
    assert DEFAULTS["init_latent"] == "none" and DEFAULTS["init_strength"] == 0.9


# ---------------------------------------------------------------------------------------------------------------- references and C ABI
def test_gradient_reference_is_the_recipe():
    u = R.gradient_u8("left", 2, 5)
    assert u.dtype == np.uint8 and u.tolist() == [[255, 191, 127, 63, 0]] * 2          # 191.25, 127.5, 63.75 truncated
    assert R.gradient_u8("right", 1, 3).tolist() == [[0, 127, 255]] and R.gradient_u8("top", 3, 1).tolist() == [[255], [127], [0]]
    assert R.gradient_u8("bottom", 1, 4).tolist() == [[0] * 4] and R.gradient_u8("top", 1, 1).tolist() == [[255]]
    img = R.gradient_image("right", 4, 6)
    assert img.shape == (3, 4, 6) and img.dtype == np.float32 and np.array_equal(img[0], img[2])
    want = R.gradient_u8("right", 4, 6) / 127.0 - 1.0           # what the VAE is to see: note 127, not 127.5
    assert np.abs((2 * img[1].astype(np.float64) - 1) - want).max() < 2e-7


def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH, parse_header
    if not os.path.exists(LIB_PATH):
        g.build()
    sig = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("tcl_light_gradient_f32", 5), ("tcl_light_start_f16", 10)):
        assert name in sig and len(sig[name][1]) == nargs and hasattr(dll, name), name
    assert sig["tcl_light_start_f16"][1][2] is ctypes.c_int64 and sig["tcl_light_start_f16"][1][7] is ctypes.c_float
