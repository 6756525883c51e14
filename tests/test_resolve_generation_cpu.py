"""CPU: hostlogic.resolve_generation, the one resolution of the generation options that run.py (before a model is loaded) and Generator share --
it agrees with a Generator built on the stand-in UNet of the host tests, for the defaults and for every feature switched on alone, and reports two
faults at once the way the REFUSED table of test_sweep_host_cpu.py expects."""
from types import SimpleNamespace

import pytest
import torch

from tc_light_amd import hostlogic as HL
from test_sweep_host_cpu import PATH, REFUSED

FEATURES = [dict(),
            dict(init_latent="Left", init_strength=0.5, n_timesteps=2),
            dict(init_latent="source", init_strength=1),
            dict(highres_scale=1.5, highres_denoise=0.25),
            dict(iclight_model="FBC", bg_source="Grey"),
            dict(iclight_model="fbc", fbc_matting=False),
            dict(light_path=[(0, 0), (1, 180)], init_strength=0.5, n_timesteps=2),
            dict(light_path=[[0, 0], [1, 540]], iclight_model="fbc"),
            dict(normal=True, iclight_model="fbc"),
            dict(normal=True, iclight_model="fbc", apply_opt=False, fbc_matting=False),
            dict(prompt_path=[(0, "sunrise"), (1, "dusk")]),
            dict(noise_mode="vanilla", alpha_t=0.3),
            dict(background_cond=True)]
DERIVED = ("fbc", "light", "img2img", "highres", "normal_sides", "schedule", "schedule_highres")


def _stub():
    return SimpleNamespace(dev=torch.device("cpu"), tome=SimpleNamespace(args={}))


@pytest.mark.parametrize("keys", FEATURES, ids=lambda k: "+".join(k) or "defaults")
def test_agrees_with_the_stand_in_generator(keys):
    from tc_light_amd.generate import DEFAULTS, Generator
    before = dict(DEFAULTS, **keys)
    r = HL.resolve_generation(dict(before))
    assert sorted(r) == sorted(HL.RESOLVED_KEYS + DERIVED)
    g = Generator(_stub(), None, dict(keys, max_tokens_per_pass=1))
    for k in HL.RESOLVED_KEYS:
        assert getattr(g.cfg, k) == r[k] and type(getattr(g.cfg, k)) is type(r[k]), k
    for k in DERIVED:
        assert getattr(g, k) == r[k], k
    # the values, spelled out: what each check_* returns on its own, and what follows from them
    n = before["n_timesteps"]
    assert (r["init_latent"], r["init_strength"]) == HL.check_init(before["init_latent"], before["init_strength"], n)
    assert (r["highres_scale"], r["highres_denoise"]) == HL.check_highres(before["highres_scale"], before["highres_denoise"], n)
    assert (r["iclight_model"], r["bg_source"]) == HL.check_fbc(before["iclight_model"], before["bg_source"])
    assert r["fbc"] == (str(before["iclight_model"]).lower() == "fbc") and r["light"] == (before["light_path"] is not None)
    assert r["highres"] == (before["highres_scale"] != 1.0) and r["normal_sides"] == (HL.NORMAL_SIDES if before["normal"] else ())
    assert r["img2img"] == (r["init_latent"] != "none" or (r["light"] and not r["fbc"]))
    assert r["schedule"] == (HL.img2img_schedule(n, r["init_strength"]) if r["img2img"] else (n, 0, n))
    assert r["schedule_highres"] == (HL.img2img_schedule(n, r["highres_denoise"]) if r["highres"] else None)
    if not keys:
        assert r == dict(init_latent="none", init_strength=0.9, highres_scale=1.0, highres_denoise=0.5, iclight_model="fc", bg_source="upload",
                         light_path=None, prompt_path=None, fbc=False, light=False, img2img=False, highres=False, normal_sides=(),
                         schedule=(25, 0, 25), schedule_highres=None)


@pytest.mark.parametrize("keys,word", REFUSED)
def test_two_faults_at_once(keys, word):
    """light_path beside a key it does not combine with -- among them normal under fc, which check_normal refuses too, and a ramp bg_source under
    fbc: the message is the one that names light_path, from run.py and from Generator alike."""
    from tc_light_amd.generate import DEFAULTS, Generator
    with pytest.raises(ValueError, match=word):
        HL.resolve_generation(dict(DEFAULTS, light_path=PATH, **keys))
    with pytest.raises(ValueError, match=word):
        Generator(_stub(), None, dict(keys, light_path=PATH, max_tokens_per_pass=1))


def test_the_order_is_run_py_s():
    """check_init, check_highres, check_fbc, check_light_path, check_normal, check_prompt_path: of two faults the earlier check's is raised."""
    from tc_light_amd.generate import DEFAULTS
    for keys, word in ((dict(init_latent="diagonal", highres_scale=5.0), "init_latent"),
                       (dict(highres_scale=5.0, iclight_model="fcb"), "highres_scale"),
                       (dict(highres_scale=1.5, background_cond=True, iclight_model="fbc"), "(?s)background_cond.*highres_scale > 1"),
                       (dict(iclight_model="fbc", init_latent="left", light_path=PATH), "(?s)fbc.*init_latent"),
                       (dict(light_path=[[0.5, 0]], normal=True), "light_path positions"),
                       (dict(normal=True, prompt_path=[[0, "a"]]), "(?s)generation.normal needs.*iclight_model"),
                       (dict(normal=True, iclight_model="fbc", prompt_path=[[0, "a"]]), "(?s)prompt_path.*normal")):
        with pytest.raises(ValueError, match=word):
            HL.resolve_generation(dict(DEFAULTS, **keys))
