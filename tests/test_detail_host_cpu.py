"""Host side of generation.detail_transfer: hostlogic.check_detail's refusals, each by the name of its key; the Generator on the stand-in UNet of the
host tests; run.resolve_options (before any model is loaded); the CLI keys and the example config; resolve_generation's result, unchanged."""
import os

import pytest
import torch

from tc_light_amd import hostlogic as HL
from test_resolve_generation_cpu import DERIVED, _stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(sigma=3.0, mode="add", blend=1.0, channels="rgb")


def test_off_bare_number_and_defaults():
    assert HL.check_detail(None) is None
    assert HL.check_detail(None, normal=True, iclight_model="fbc", fbc_matting=False) is None      # off: nothing else is looked at
    assert HL.check_detail(2) == dict(FULL, sigma=2.0) and type(HL.check_detail(2)["sigma"]) is float
    assert HL.check_detail(0.5) == dict(FULL, sigma=0.5) and HL.check_detail(16) == dict(FULL, sigma=16.0)
    assert HL.check_detail({}) == FULL == HL.DETAIL_DEFAULTS
    assert HL.check_detail(dict(mode="Ratio", channels="LUMA", blend=0, sigma=1)) == dict(sigma=1.0, mode="ratio", blend=0.0, channels="luma")
    assert HL.check_detail(dict(blend=0.5), iclight_model="fbc", fbc_matting=True) == dict(FULL, blend=0.5)


@pytest.mark.parametrize("block,key", [("add", "generation.detail_transfer"), ([3.0], "generation.detail_transfer"), (True, "generation.detail_transfer"),
                                       (dict(sigma=3, radius=9), "generation.detail_transfer"), (dict(strength=1), "generation.detail_transfer"),
                                       (0.4, "generation.detail_transfer.sigma"), (16.5, "generation.detail_transfer.sigma"),
                                       (dict(sigma="3"), "generation.detail_transfer.sigma"), (dict(sigma=True), "generation.detail_transfer.sigma"),
                                       (dict(sigma=float("nan")), "generation.detail_transfer.sigma"), (dict(sigma=None), "generation.detail_transfer.sigma"),
                                       (dict(blend=-0.1), "generation.detail_transfer.blend"), (dict(blend=1.1), "generation.detail_transfer.blend"),
                                       (dict(blend="1"), "generation.detail_transfer.blend"), (dict(blend=float("nan")), "generation.detail_transfer.blend"),
                                       (dict(mode="mul"), "generation.detail_transfer.mode"), (dict(mode=1), "generation.detail_transfer.mode"),
                                       (dict(channels="hsv"), "generation.detail_transfer.channels"), (dict(channels=None), "generation.detail_transfer.channels")])
def test_refuses_malformed(block, key):
    with pytest.raises(ValueError) as e:
        HL.check_detail(block)
    assert key in str(e.value) and (key.count(".") == 1 or key + " " in str(e.value))


def test_refuses_normal_and_fbc_without_matting():
    with pytest.raises(ValueError) as e:
        HL.check_detail(3.0, normal=True, iclight_model="fbc")
    assert "generation.detail_transfer" in str(e.value) and "generation.normal" in str(e.value)
    with pytest.raises(ValueError) as e:
        HL.check_detail(3.0, iclight_model="FBC", fbc_matting=False)
    assert all(w in str(e.value) for w in ("generation.detail_transfer", "generation.iclight_model fbc", "generation.fbc_matting"))
    assert HL.check_detail(3.0, iclight_model="fc", fbc_matting=False) == FULL      # fc: the matte plays no part


# ---------------------------------------------------------------------------------------------------------------- the Generator
def test_generator_normalises_and_refuses():
    from tc_light_amd.generate import DEFAULTS, Generator
    assert DEFAULTS["detail_transfer"] is None
    g = Generator(_stub(), None, dict(max_tokens_per_pass=1))
    assert g.cfg.detail_transfer is None and g.fbc_alpha is None
    g = Generator(_stub(), None, dict(max_tokens_per_pass=1, detail_transfer=2))
    assert g.cfg.detail_transfer == dict(FULL, sigma=2.0)
    for keys, words in ((dict(detail_transfer=dict(mode="mul")), ["generation.detail_transfer.mode"]),
                        (dict(detail_transfer=3.0, normal=True, iclight_model="fbc"), ["generation.detail_transfer", "generation.normal"]),
                        (dict(detail_transfer=3.0, iclight_model="fbc", fbc_matting=False), ["generation.detail_transfer", "generation.fbc_matting"])):
        with pytest.raises(ValueError) as e:
            Generator(_stub(), None, dict(keys, max_tokens_per_pass=1))
        assert all(w in str(e.value) for w in words)


class _Vae:
    def encode_imgs_batch(self, images, bs):
        return torch.zeros(images.shape[0], 4, images.shape[-2] // 8, images.shape[-1] // 8, dtype=torch.float16)

    def decode_latents_batch(self, x, bs):
        return torch.full((x.shape[0], 3, 8 * x.shape[-2], 8 * x.shape[-1]), 0.25)


def _stand_in_call(monkeypatch, **keys):
    """Generator.__call__ on the stand-in UNet with the denoise cut out: what surrounds the step, on the CPU."""
    from tc_light_amd import generate as G
    monkeypatch.setattr(G, "lib", lambda: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: None)
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda dev=None: 0)
    g = G.Generator(_stub(), _Vae(), dict(keys, max_tokens_per_pass=1, apply_opt=False, n_timesteps=1))
    monkeypatch.setattr(g, "ddim_sample", lambda x, *a, **k: x)
    frames = torch.rand(2, 3, 16, 16)
    conds = torch.zeros(2, 77, 768, dtype=torch.float16)
    return g, frames, conds


def test_stand_in_generator_with_the_key_off_has_no_detail_entry(monkeypatch):
    g, frames, conds = _stand_in_call(monkeypatch)
    out, info = g(frames, conds, conds, None, None, None)
    assert "detail" not in info and "detail" not in info["timing"] and "detail" not in g.timing
    assert sorted(info["timing"]) == ["decode", "denoise", "encode", "stage1", "stage2", "total"] and tuple(out.shape) == (2, 3, 16, 16)
    g, frames, conds = _stand_in_call(monkeypatch, detail_transfer=dict(blend=0))      # blend 0: nothing runs, no source is asked for
    out0, info = g(frames, conds, conds, None, None, None)
    assert "detail" not in info and "detail" not in info["timing"] and torch.equal(out0, out)


def test_stand_in_generator_hands_the_step_its_frames(monkeypatch):
    from tc_light_amd import detail
    seen = {}

    def fake(source, relit, sigma, mode, blend, channels, mask=None):
        seen.update(source=source, relit=relit, args=(sigma, mode, blend, channels), mask=mask)
        return relit + 1
    monkeypatch.setattr(detail, "detail_transfer", fake)
    g, frames, conds = _stand_in_call(monkeypatch, detail_transfer=dict(sigma=1, mode="ratio", blend=0.5, channels="luma"))
    with pytest.raises(ValueError, match="generation.detail_transfer: source"):
        g(frames, conds, conds, None, None, None)
    with pytest.raises(ValueError, match="generation.detail_transfer: source"):
        g(frames, conds, conds, None, None, None, source=frames[:1])
    out, info = g(frames, conds, conds, None, None, None, source=frames)
    assert torch.equal(seen["source"], frames) and seen["args"] == (1.0, "ratio", 0.5, "luma") and seen["mask"] is None
    assert torch.equal(out, seen["relit"] + 1) and float(seen["relit"].mean()) == 0.25      # the step ran last, on the decoded frames
    assert info["detail"] == dict(sigma=1.0, mode="ratio", blend=0.5, channels="luma") and info["timing"]["detail"] >= 0
    assert info["timing"]["total"] >= info["timing"]["detail"] and info["total_time"] == info["timing"]["total"]


# ---------------------------------------------------------------------------------------------------------------- run.py, the CLI, the example
def _run_cfg(tmp_path, generation):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}, {generation}}}
""")
    return str(cfg)


@pytest.mark.parametrize("generation,flags,words", [
    ("detail_transfer: {sigma: 20}", [], ["generation.detail_transfer.sigma"]),
    ("detail_transfer: {sigma: 3, taps: 5}", [], ["generation.detail_transfer"]),
    ("detail_transfer: 3, normal: true, iclight_model: fbc, bg_source: left", [], ["generation.detail_transfer", "generation.normal"]),
    ("iclight_model: fbc, bg_source: left, fbc_matting: false", ["--detail"], ["generation.detail_transfer", "generation.fbc_matting"]),
    ("alpha_t: 0.0", ["--detail", "0.1"], ["generation.detail_transfer.sigma"]),
    ("alpha_t: 0.0", ["--detail_blend", "2"], ["generation.detail_transfer.blend"])])
def test_run_refuses_before_models(tmp_path, monkeypatch, generation, flags, words):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.detail_transfer was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    with pytest.raises(ValueError) as e:
        run.main(["--config", _run_cfg(tmp_path, generation)] + flags)
    assert all(w in str(e.value) for w in words)


def test_run_reaches_the_models_with_a_good_block(tmp_path, monkeypatch):
    import run
    from tc_light_amd.config_utils import load_config

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached
    monkeypatch.setattr(run, "init_iclight", stop)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)
    with pytest.raises(Reached):
        run.main(["--config", _run_cfg(tmp_path, "detail_transfer: 2"), "--detail_mode", "ratio"])
    config = load_config(["--config", _run_cfg(tmp_path, "detail_transfer: 2"), "--detail_mode", "ratio"], print_config=False)
    o = run.resolve_options(config)
    assert o.detail == dict(FULL, sigma=2.0, mode="ratio") == dict(config.generation.detail_transfer)      # what config.yaml records
    config = load_config(["--config", _run_cfg(tmp_path, "alpha_t: 0.0")], print_config=False)
    assert run.resolve_options(config).detail is None and config.generation.detail_transfer is None


def test_cli_sets_the_keys():
    from tc_light_amd.config_utils import DEFAULTS, load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        base = os.path.join("configs", "tclight_default.yaml")
        d = load_config(["--config", base], print_config=False)
        e = load_config(["--config", base, "--detail"], print_config=False)
        f = load_config(["--config", base, "--detail", "2", "--detail_mode", "ratio", "--detail_blend", "0.5"], print_config=False)
        h = load_config(["--config", base, "--detail_blend", "0.5"], print_config=False)
        x = load_config(["--config", os.path.join("configs", "examples", "tclight_detail.yaml")], print_config=False)
    finally:
        os.chdir(cwd)
    assert d.generation.detail_transfer is None and DEFAULTS["generation"]["detail_transfer"] is None
    assert dict(e.generation.detail_transfer) == dict(sigma=3.0) and dict(h.generation.detail_transfer) == dict(blend=0.5)
    assert dict(f.generation.detail_transfer) == dict(sigma=2.0, mode="ratio", blend=0.5)
    assert HL.check_detail(dict(x.generation.detail_transfer)) == FULL and x.generation.alpha_t == 0.01 and x.models.unet


def test_resolve_generation_is_unchanged():
    """The key is the caller's check, as ip_adapter is: resolve_generation neither reads nor returns it."""
    from tc_light_amd.generate import DEFAULTS
    assert "detail_transfer" not in HL.RESOLVED_KEYS
    r = HL.resolve_generation(dict(DEFAULTS, detail_transfer="not even looked at"))
    assert sorted(r) == sorted(HL.RESOLVED_KEYS + DERIVED)
    assert r == HL.resolve_generation({k: v for k, v in DEFAULTS.items() if k != "detail_transfer"})
    assert r == dict(init_latent="none", init_strength=0.9, highres_scale=1.0, highres_denoise=0.5, iclight_model="fc", bg_source="upload",
                     light_path=None, prompt_path=None, fbc=False, light=False, img2img=False, highres=False, normal_sides=(),
                     schedule=(25, 0, 25), schedule_highres=None)


def test_invert_ignores_the_key():
    for name in ("invert.py", os.path.join("tc_light_amd", "invert.py")):
        with open(os.path.join(ROOT, name)) as f:
            assert "detail_transfer" not in f.read()
