"""generation.fullres on the CPU: the derived bound pinned from both sides (the f32 emulation of the kernel's sequence lies inside it, three planted
defects outside it, on the same inputs); the crop geometry against process_frames; hostlogic.check_fullres, every refusal by name; the CLI keys, the
example config and run.resolve_options before any model is loaded; a run without the key resolves to what it did."""
import os

import numpy as np
import pytest
import torch

import fullres_refs as R
from tc_light_amd import hostlogic as HL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(radius=8, eps=1e-3, guide="rgb")


# ---------------------------------------------------------------------------------------------------------------- the bound, from both sides
def _worst(got, c):
    ea = np.abs(got[0].astype(np.float64) - c["abar"]) / c["e_abar"]
    eb = np.abs(got[1].astype(np.float64) - c["bbar"]) / c["e_bbar"]
    return max(ea.max(), eb.max())


@pytest.mark.parametrize("guide,eps", R.FIT_SETTINGS)
@pytest.mark.parametrize("name", sorted(R.fit_geometries()))
def test_emulation_inside_the_bound_and_defects_outside(name, guide, eps):
    c = R.fit_case(name, guide, eps, N=1)
    inside = _worst(R.emulate_fit_f32(c["S"], c["R"], c["r"], eps, guide), c)
    no_clip = _worst(R.emulate_fit_f32(c["S"], c["R"], c["r"], eps, guide, unclipped_count=True), c)
    no_mean = _worst(R.emulate_fit_f32(c["S"], c["R"], c["r"], eps, guide, second_mean=False), c)
    print(f"{name} {guide} eps {eps}: err/bound emulation {inside:.3f}, unclipped count {no_clip:.3g}, no second mean {no_mean:.3g}; "
          f"max bound abar {c['e_abar'].max():.3e} bbar {c['e_bbar'].max():.3e}")
    assert inside <= 1.0
    assert no_clip > 1.0 and no_mean > 1.0
    assert c["e_abar"].max() < 0.05 and c["e_bbar"].max() < 0.05      # the bound says something: far below the fields' own size (a ~ 1)


def test_the_bound_scales_like_one_over_eps_on_a_flat_guide():
    """var = 0 everywhere: the denominator is eps alone and e_a = e_cov / eps, so a tenth of the eps gives ten times the bound on a."""
    S = np.full((1, 3, 12, 12), 0.75, np.float32)
    Rl = np.random.default_rng(0).random((1, 3, 12, 12)).astype(np.float32)
    lo, hi = R.fit_bound(S, Rl, 2, 1e-3, "rgb")[0], R.fit_bound(S, Rl, 2, 1e-2, "rgb")[0]
    ratio = lo / hi
    assert 9.0 < ratio.min() and ratio.max() < 10.5


@pytest.mark.parametrize("name", sorted(R.APPLY_CASES))
def test_apply_emulation_matches_and_align_corners_does_not(name):
    abar, bbar, src = R.apply_inputs(name)
    ok, bad, near = R.apply_matches(R.emulate_apply_f32(abar, bbar, src), abar, bbar, src)
    print(f"{name}: emulation mismatches {bad}, share of values within the bound of a rounding boundary {near:.2e}")
    assert ok and near < 0.01
    if abar.shape[-1] > 1:                                       # one field pixel: both samplings read the same value
        ok, bad, _ = R.apply_matches(R.emulate_apply_f32(abar, bbar, src, align_corners=True), abar, bbar, src)
        assert not ok and bad > 0.05 * src.size


def test_apply_identity_and_reference_definition():
    abar, bbar, src = R.apply_inputs("13to37")
    one, zero = np.ones_like(abar), np.zeros_like(bbar)
    assert np.array_equal(R.emulate_apply_f32(one, zero, src), src) and np.array_equal(R.apply_reference(one, zero, src)[1], src)
    # the half-pixel coordinates, restated: output 0 of 13 -> 37 sits at (0 + 0.5) * 13 / 37 - 0.5 < 0, clamped to 0; the last at 12 (clamped)
    i0, i1, f = R._coords(37, 13)
    assert i0[0] == 0 and f[0] == 0.0 and i0[-1] == 12 and i1[-1] == 12 and f[-1] == 0.0
    assert abs((i0 + f)[18] - ((18 + 0.5) * 13 / 37 - 0.5)) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- geometry
SIZES = [((2160, 3840), (720, 1280)), ((1080, 1920), (720, 1280)), ((1081, 1921), (720, 1280)), ((479, 853), (64, 64)), ((853, 479), (64, 64)),
         ((131, 257), (64, 96)), ((257, 131), (96, 64)), ((1000, 999), (333, 500)), ((77, 301), (24, 100)), ((128, 128), (64, 64)),
         ((129, 127), (64, 64)), ((4320, 7680), (1088, 1920)), ((65, 65), (64, 64))]


@pytest.mark.parametrize("native,work", SIZES)
def test_geometry_agrees_with_process_frames(native, work):
    from tc_light_amd import fullres
    from tc_light_amd.dataparser import process_frames
    (H0, W0), (h, w) = native, work
    g = fullres.geometry(H0, W0, h, w)
    assert g == R.geometry(H0, W0, h, w)
    assert g["s"] == max(w / W0, h / H0) < 1 and (g["nh"], g["nw"]) == (int(round(H0 * g["s"])), int(round(W0 * g["s"])))
    # the crop lies inside the frame and resizing it with process_frames gives the working frame's extent
    assert 0 <= g["X0"] and 0 <= g["Y0"] and g["X0"] + g["Wc"] <= W0 and g["Y0"] + g["Hc"] <= H0 and g["Hc"] >= h and g["Wc"] >= w
    ramp = torch.arange(W0, dtype=torch.float32)[None, None, None, :].expand(1, 1, H0, W0) / W0 + \
        torch.arange(H0, dtype=torch.float32)[None, None, :, None] / H0 * 2.0
    whole = process_frames(ramp, h, w)
    crop = process_frames(ramp[..., g["Y0"]:g["Y0"] + g["Hc"], g["X0"]:g["X0"] + g["Wc"]], h, w)
    assert tuple(whole.shape[-2:]) == tuple(crop.shape[-2:]) == (h, w)
    # the same picture: a ramp resized either way agrees to within the rounding of the crop (one working pixel on each axis)
    assert float((whole - crop).abs().max()) <= 1.0 / w + 2.0 / h + 1e-6
    # the crop covers the working frame's share of the native one to within a native pixel
    assert abs(g["Wc"] - w / g["s"]) <= 1.0 and abs(g["Hc"] - h / g["s"]) <= 1.0


@pytest.mark.parametrize("native,work", [((64, 64), (64, 64)), ((720, 1280), (720, 1280)), ((60, 300), (64, 64)), ((64, 1000), (64, 64)),
                                         ((32, 32), (64, 64))])
def test_a_source_that_is_not_larger_is_refused_with_the_sizes(native, work):
    from tc_light_amd import fullres
    with pytest.raises(ValueError) as e:
        fullres.geometry(*native, *work)
    assert "generation.fullres" in str(e.value) and f"{native[0]}x{native[1]}" in str(e.value) and f"{work[0]}x{work[1]}" in str(e.value)


def test_batch_size_keeps_the_cap_whatever_the_length():
    from tc_light_amd import fullres
    per = fullres.bytes_per_frame(720, 1280, 2160, 3840)
    assert per == 2 * 3 * 2160 * 3840 + 24 * 720 * 1280 + fullres.WS_PLANES * 4 * 720 * 1280
    B = fullres.batch_size(720, 1280, 2160, 3840)
    assert B >= 1 and B * per <= fullres.CAP_BYTES < (B + 1) * per
    assert fullres.batch_size(720, 1280, 2160, 3840, cap_bytes=1) == 1                       # one frame at least
    assert fullres.batch_size(8, 8, 16, 16) * fullres.WS_PLANES * 64 < 2 ** 31            # no more than one fit call takes


def test_native_u8_is_the_cached_read(tmp_path, monkeypatch):
    from tc_light_amd import dataparser as D
    u8 = np.random.default_rng(1).integers(0, 256, (3, 10, 14, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", u8)
    p = D.VideoDataParser(dict(rgb_path=str(tmp_path / "clip.npy"), height=8, width=8), "cpu")
    p.load_video([0, 2])
    monkeypatch.setattr(D, "read_frames", lambda path: (_ for _ in ()).throw(AssertionError("the file was read a second time")))
    assert p.native_size() == (10, 14)
    got = p.native_u8([0, 2])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 10, 14, 3) and np.array_equal(got.numpy(), u8[[0, 2]])


# ---------------------------------------------------------------------------------------------------------------- options
def test_off_true_bare_radius_and_defaults():
    assert HL.check_fullres(None) is None and HL.check_fullres(False) is None
    assert HL.check_fullres(None, normal=True, iclight_model="fbc", background_cond=True, scene_type="sceneflow") is None      # off: nothing else is looked at
    assert HL.check_fullres(True) == FULL == HL.FULLRES_DEFAULTS == HL.check_fullres({})
    assert HL.check_fullres(4) == dict(FULL, radius=4) and HL.check_fullres(1)["radius"] == 1 and HL.check_fullres(64)["radius"] == 64
    assert HL.check_fullres(dict(eps=1, guide="LUMA")) == dict(radius=8, eps=1.0, guide="luma") and type(HL.check_fullres(dict(eps=1))["eps"]) is float
    assert HL.check_fullres(dict(eps=1e-4))["eps"] == 1e-4
    assert HL.check_fullres(HL.check_fullres(True)) == FULL                                  # the normalised block passes again (the Generator re-checks it)


@pytest.mark.parametrize("block,key", [("on", "generation.fullres"), ([8], "generation.fullres"), (8.0, "generation.fullres"),
                                       (dict(radius=8, sigma=3), "generation.fullres"), (dict(blend=1), "generation.fullres"),
                                       (0, "generation.fullres.radius"), (65, "generation.fullres.radius"), (dict(radius=8.0), "generation.fullres.radius"),
                                       (dict(radius=True), "generation.fullres.radius"), (dict(radius=None), "generation.fullres.radius"),
                                       (dict(eps=9e-5), "generation.fullres.eps"), (dict(eps=1.01), "generation.fullres.eps"),
                                       (dict(eps="1e-3"), "generation.fullres.eps"), (dict(eps=float("nan")), "generation.fullres.eps"),
                                       (dict(eps=True), "generation.fullres.eps"), (dict(guide="hsv"), "generation.fullres.guide"),
                                       (dict(guide=1), "generation.fullres.guide"), (dict(guide=None), "generation.fullres.guide")])
def test_refuses_malformed(block, key):
    with pytest.raises(ValueError) as e:
        HL.check_fullres(block)
    assert key in str(e.value) and (key.count(".") == 1 or key + " " in str(e.value))


@pytest.mark.parametrize("keys,words", [(dict(normal=True), ["generation.fullres", "generation.normal"]),
                                        (dict(iclight_model="FBC"), ["generation.fullres", "generation.iclight_model fbc"]),
                                        (dict(background_cond=True), ["generation.fullres", "generation.background_cond"]),
                                        (dict(scene_type="SceneFlow"), ["generation.fullres", "data.scene_type sceneflow", "out of scope"])])
def test_refuses_what_it_does_not_combine_with(keys, words):
    with pytest.raises(ValueError) as e:
        HL.check_fullres(True, **keys)
    assert all(w in str(e.value) for w in words)


def test_null_leaves_the_resolved_options_of_a_plain_run_as_they_are():
    from tc_light_amd.generate import DEFAULTS
    assert DEFAULTS["fullres"] is None and "fullres" not in HL.RESOLVED_KEYS
    plain = HL.resolve_generation({k: v for k, v in DEFAULTS.items() if k != "fullres"})
    assert HL.resolve_generation(dict(DEFAULTS)) == plain == HL.resolve_generation(dict(DEFAULTS, fullres=False)) and "fullres" not in plain
    assert plain == dict(init_latent="none", init_strength=0.9, highres_scale=1.0, highres_denoise=0.5, iclight_model="fc", bg_source="upload",
                         light_path=None, prompt_path=None, fbc=False, light=False, img2img=False, highres=False, normal_sides=(),
                         schedule=(25, 0, 25), schedule_highres=None)
    on = HL.resolve_generation(dict(DEFAULTS, fullres=dict(guide="luma")))
    assert on.pop("fullres") == dict(FULL, guide="luma") and on == plain
    with pytest.raises(ValueError, match="generation.fullres.radius"):
        HL.resolve_generation(dict(DEFAULTS, fullres=0))
    with pytest.raises(ValueError, match="(?s)generation.fullres.*sceneflow"):
        HL.resolve_generation(dict(DEFAULTS, fullres=True, scene_type="sceneflow"))


def test_generator_checks_the_key_with_the_others():
    from tc_light_amd.generate import Generator
    from test_resolve_generation_cpu import _stub
    assert Generator(_stub(), None, dict(max_tokens_per_pass=1)).cfg.fullres is None
    assert Generator(_stub(), None, dict(max_tokens_per_pass=1, fullres=4)).cfg.fullres == dict(FULL, radius=4)
    with pytest.raises(ValueError, match="generation.fullres.eps"):
        Generator(_stub(), None, dict(max_tokens_per_pass=1, fullres=dict(eps=2)))


# ---------------------------------------------------------------------------------------------------------------- run.py, the CLI, the example
def _run_cfg(tmp_path, generation, data="height: 64, width: 64"):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{{data}}}
generation: {{prompt: {{edit: "warm light"}}, {generation}}}
""")
    return str(cfg)


@pytest.mark.parametrize("generation,data,flags,words", [
    ("fullres: {radius: 70}", None, [], ["generation.fullres.radius"]),
    ("fullres: {radius: 8, taps: 5}", None, [], ["generation.fullres"]),
    ("alpha_t: 0.0", None, ["--fullres", "0"], ["generation.fullres.radius"]),
    ("alpha_t: 0.0", None, ["--fullres_eps", "2"], ["generation.fullres.eps"]),
    ("fullres: true, normal: true, iclight_model: fbc, bg_source: left", None, [], ["generation.fullres", "generation.normal"]),
    ("iclight_model: fbc, bg_source: left", None, ["--fullres"], ["generation.fullres", "generation.iclight_model fbc"]),
    ("fullres: 4", "height: 64, width: 64, scene_type: sceneflow", [], ["generation.fullres", "data.scene_type sceneflow"])])
def test_run_refuses_before_models(tmp_path, monkeypatch, generation, data, flags, words):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.fullres was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    with pytest.raises(ValueError) as e:
        run.main(["--config", _run_cfg(tmp_path, generation, data or "height: 64, width: 64")] + flags)
    assert all(w in str(e.value) for w in words)


def test_run_resolves_and_records_the_block(tmp_path):
    import run
    from tc_light_amd.config_utils import load_config
    config = load_config(["--config", _run_cfg(tmp_path, "fullres: 4"), "--fullres_guide", "luma"], print_config=False)
    o = run.resolve_options(config)
    assert o.fullres == dict(FULL, radius=4, guide="luma") == dict(config.generation.fullres)      # what config.yaml records
    config = load_config(["--config", _run_cfg(tmp_path, "alpha_t: 0.0")], print_config=False)
    assert run.resolve_options(config).fullres is None and config.generation.fullres is None


def test_cli_sets_the_keys_and_the_example_loads():
    from tc_light_amd.config_utils import DEFAULTS, load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        base = os.path.join("configs", "tclight_default.yaml")
        d = load_config(["--config", base], print_config=False)
        e = load_config(["--config", base, "--fullres"], print_config=False)
        f = load_config(["--config", base, "--fullres", "4", "--fullres_eps", "0.01", "--fullres_guide", "luma"], print_config=False)
        h = load_config(["--config", base, "--fullres_eps", "0.01"], print_config=False)
        x = load_config(["--config", os.path.join("configs", "examples", "tclight_fullres.yaml")], print_config=False)
    finally:
        os.chdir(cwd)
    assert d.generation.fullres is None and DEFAULTS["generation"]["fullres"] is None
    assert dict(e.generation.fullres) == dict(radius=8) and dict(h.generation.fullres) == dict(eps=0.01)
    assert dict(f.generation.fullres) == dict(radius=4, eps=0.01, guide="luma")
    assert HL.check_fullres(dict(x.generation.fullres)) == FULL and x.models.unet
