"""Host side of generation.ip_adapter: the adapter file's loader (index -> block map, shape checks, the refused 'plus' files, both file formats),
hostlogic.check_ip_adapter's refusals, their place in run.main (before any model is loaded), the CLI keys and the example config."""
import os

import pytest
import torch

from tc_light_amd import hostlogic as HL
from tc_light_amd import ip_adapter as IP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def state():
    return IP.seeded_state_dict(3)


# ---------------------------------------------------------------------------------------------------------------- loader
def test_index_to_block_map():
    m = IP.BLOCK_OF_INDEX
    assert sorted(m) == list(range(1, 32, 2)) and len(set(m.values())) == 16
    assert m[1] == "down_blocks.0.attentions.0." and m[3] == "down_blocks.0.attentions.1." and m[11] == "down_blocks.2.attentions.1."
    assert m[13] == "up_blocks.1.attentions.0." and m[17] == "up_blocks.1.attentions.2." and m[29] == "up_blocks.3.attentions.2."
    assert m[31] == "mid_block.attentions.0."
    w = IP.block_widths()
    widths = {i: w[p] for i, p in m.items()}
    assert [widths[i] for i in range(1, 32, 2)] == [320, 320, 640, 640, 1280, 1280] + [1280] * 3 + [640] * 3 + [320] * 3 + [1280]
    from tc_light_amd import sd15
    blocks = {k[:-len("proj_in.weight")] for k in sd15.unet_param_shapes() if k.endswith("proj_in.weight")}
    assert set(m.values()) == blocks                             # every transformer block of the engine gets one pair


def test_check_state_maps_every_block(state):
    proj, weights = IP.check_state(state)
    assert tuple(proj["weight"].shape) == (3072, 1024) and tuple(proj["norm_weight"].shape) == (768,)
    for i, p in IP.BLOCK_OF_INDEX.items():
        C = IP.block_widths()[p]
        assert tuple(weights[p].shape) == (2 * C, 768)
        assert torch.equal(weights[p][:C], state[f"ip_adapter.{i}.to_k_ip.weight"]) and torch.equal(weights[p][C:], state[f"ip_adapter.{i}.to_v_ip.weight"])


def test_swapped_indices_of_different_width_raise(state):
    sd = dict(state)
    for kind in ("to_k_ip", "to_v_ip"):                          # 3 (320) <-> 5 (640)
        sd[f"ip_adapter.3.{kind}.weight"], sd[f"ip_adapter.5.{kind}.weight"] = state[f"ip_adapter.5.{kind}.weight"], state[f"ip_adapter.3.{kind}.weight"]
    with pytest.raises(ValueError, match=r"ip_adapter\.3\.to_k_ip\.weight") as e:
        IP.check_state(sd)
    assert "(640, 768)" in str(e.value) and "(320, 768)" in str(e.value)


def test_missing_index_raises(state):
    sd = {k: v for k, v in state.items() if not k.startswith("ip_adapter.31.")}
    with pytest.raises(ValueError, match=r"ip_adapter\.31\.to_k_ip\.weight"):
        IP.check_state(sd)


def test_plus_file_is_refused(state):
    sd = dict(state, **{"image_proj.latents": torch.zeros(1, 16, 768)})
    with pytest.raises(ValueError, match="plus"):
        IP.check_state(sd)


def test_bin_and_safetensors_both_read(tmp_path, state):
    from safetensors.torch import save_file
    st, bn = str(tmp_path / "ip-adapter_sd15.safetensors"), str(tmp_path / "ip-adapter_sd15.bin")
    save_file({k: v.contiguous() for k, v in state.items()}, st)
    torch.save(IP.to_nested(state), bn)
    for path in (st, bn):
        flat = IP.read_file(path)
        assert set(flat) == set(state) and all(torch.equal(flat[k], state[k]) for k in state)
        proj, weights = IP.load_state(path)
        assert len(weights) == 16 and torch.equal(proj["bias"], state["image_proj.proj.bias"])


def test_load_state_missing_file(tmp_path):
    with pytest.raises(FileNotFoundError, match="IP-Adapter"):
        IP.load_state(str(tmp_path / "nope.safetensors"))
    with pytest.warns(UserWarning, match="random"):
        proj, weights = IP.load_state(str(tmp_path / "nope.safetensors"), allow=True)
    assert len(weights) == 16


# ---------------------------------------------------------------------------------------------------------------- check_ip_adapter
@pytest.fixture
def files(tmp_path):
    img, ad, enc = tmp_path / "ref.png", tmp_path / "ip-adapter_sd15.safetensors", tmp_path / "image_encoder"
    img.write_bytes(b"x"); ad.write_bytes(b"x"); enc.mkdir()
    return dict(image=str(img), models=dict(ip_adapter=str(ad), image_encoder=str(enc)))


def test_check_off_and_defaults(files):
    assert HL.check_ip_adapter(None) is None
    assert HL.check_ip_adapter(None, normal=True) is None        # off: nothing else is looked at
    got = HL.check_ip_adapter(dict(image=files["image"]), False, files["models"])
    assert got == dict(image=files["image"], scale=HL.IP_SCALE_DEFAULT, path=files["models"]["ip_adapter"], image_encoder=files["models"]["image_encoder"])
    got = HL.check_ip_adapter(dict(image=files["image"], scale=2, path=files["image"]), False, files["models"])
    assert got["scale"] == 2.0 and got["path"] == files["image"]


@pytest.mark.parametrize("block,key", [("ref.png", "generation.ip_adapter"), ({}, "generation.ip_adapter"), (dict(image="x", weight=1), "generation.ip_adapter"),
                                       (dict(scale=0.5), "generation.ip_adapter.image"), (dict(image=3), "generation.ip_adapter.image"),
                                       (dict(image="IMG", scale=-0.1), "generation.ip_adapter.scale"), (dict(image="IMG", scale=2.5), "generation.ip_adapter.scale"),
                                       (dict(image="IMG", scale="1"), "generation.ip_adapter.scale"), (dict(image="IMG", scale=True), "generation.ip_adapter.scale"),
                                       (dict(image="IMG", scale=float("nan")), "generation.ip_adapter.scale"),
                                       (dict(image="IMG", path=4), "generation.ip_adapter.path"), (dict(image="MISSING"), "generation.ip_adapter.image")])
def test_check_refuses_malformed(files, block, key):
    if isinstance(block, dict) and block.get("image") == "IMG":
        block = dict(block, image=files["image"])
    with pytest.raises(ValueError) as e:
        HL.check_ip_adapter(block, False, files["models"])
    assert key in str(e.value)


def test_check_refuses_normal(files):
    with pytest.raises(ValueError) as e:
        HL.check_ip_adapter(dict(image=files["image"]), True, files["models"])
    assert "generation.ip_adapter" in str(e.value) and "generation.normal" in str(e.value)


@pytest.mark.parametrize("drop,word", [("ip_adapter", "models.ip_adapter"), ("image_encoder", "models.image_encoder")])
def test_check_missing_weights(files, drop, word):
    models = dict(files["models"], **{drop: ""})
    with pytest.raises(FileNotFoundError, match=word):
        HL.check_ip_adapter(dict(image=files["image"]), False, models)
    assert HL.check_ip_adapter(dict(image=files["image"]), False, models, allow_random=True)["scale"] == HL.IP_SCALE_DEFAULT


# ---------------------------------------------------------------------------------------------------------------- run.main, the CLI, the example
def _run_cfg(tmp_path, generation, models=""):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}, {generation}}}
{models}
""")
    return str(cfg)


@pytest.mark.parametrize("case", ["malformed", "scale", "image", "normal", "adapter", "encoder"])
def test_run_refuses_before_models(tmp_path, monkeypatch, files, case):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.ip_adapter was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    monkeypatch.delenv("TCL_ALLOW_RANDOM_WEIGHTS", raising=False)
    img, m = files["image"], files["models"]
    models = f"models: {{ip_adapter: {m['ip_adapter']}, image_encoder: {m['image_encoder']}}}"
    gen, exc, words = {
        "malformed": (f"ip_adapter: [{img}]", ValueError, ["generation.ip_adapter"]),
        "scale": (f"ip_adapter: {{image: {img}, scale: 3}}", ValueError, ["generation.ip_adapter.scale"]),
        "image": (f"ip_adapter: {{image: {img}.missing}}", ValueError, ["generation.ip_adapter.image"]),
        "normal": (f"ip_adapter: {{image: {img}}}, normal: true, iclight_model: fbc, bg_source: left", ValueError, ["generation.ip_adapter", "generation.normal"]),
        "adapter": (f"ip_adapter: {{image: {img}}}", FileNotFoundError, ["models.ip_adapter"]),
        "encoder": (f"ip_adapter: {{image: {img}}}", FileNotFoundError, ["models.image_encoder"]),
    }[case]
    if case == "adapter":
        models = f"models: {{image_encoder: {m['image_encoder']}}}"
    if case == "encoder":
        models = f"models: {{ip_adapter: {m['ip_adapter']}}}"
    with pytest.raises(exc) as e:
        run.main(["--config", _run_cfg(tmp_path, gen, models)])
    assert all(w in str(e.value) for w in words)


def test_run_reaches_the_models_with_a_good_block(tmp_path, monkeypatch, files):
    """The same configuration with nothing wrong gets as far as init_iclight: the refusals above are the check's, not an accident of the setup."""
    import run

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached
    monkeypatch.setattr(run, "init_iclight", stop)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)      # run.main picks its device before it loads the models; none is needed here
    m = files["models"]
    with pytest.raises(Reached):
        run.main(["--config", _run_cfg(tmp_path, f"ip_adapter: {{image: {files['image']}, scale: 0.5}}",
                                       f"models: {{ip_adapter: {m['ip_adapter']}, image_encoder: {m['image_encoder']}}}")])


def test_cli_sets_the_keys():
    from tc_light_amd.config_utils import DEFAULTS, load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        base = os.path.join("configs", "tclight_default.yaml")
        d = load_config(["--config", base], print_config=False)
        e = load_config(["--config", base, "--ip_image", "photo.jpg", "--ip_scale", "0.8"], print_config=False)
        f = load_config(["--config", base, "--ip_image", "photo.jpg"], print_config=False)
    finally:
        os.chdir(cwd)
    assert d.generation.ip_adapter is None and DEFAULTS["generation"]["ip_adapter"] is None
    assert dict(e.generation.ip_adapter) == dict(image="photo.jpg", scale=0.8) and dict(f.generation.ip_adapter) == dict(image="photo.jpg")
    assert "ip_adapter" in d.models and "image_encoder" in d.models and set(DEFAULTS["models"]) == {"ip_adapter", "image_encoder"}


def test_example_config_loads():
    from tc_light_amd.config_utils import load_config
    from tc_light_amd.generate import DEFAULTS
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_ip_adapter.yaml")], print_config=False)
    finally:
        os.chdir(cwd)
    ip = c.generation.ip_adapter
    assert set(ip) == {"image", "scale", "path"} and ip["scale"] == 0.6 and ip["path"] is None and c.generation.alpha_t == 0.01
    assert c.models.ip_adapter.endswith("ip-adapter_sd15.safetensors") and c.models.image_encoder and c.models.unet      # the base's models are kept
    assert DEFAULTS["ip_adapter"] is None


def test_invert_ignores_the_key():
    """invert.py reads no generation.ip_adapter: the inversion is the plain UNet's."""
    for name in ("invert.py", os.path.join("tc_light_amd", "invert.py")):
        with open(os.path.join(ROOT, name)) as f:
            assert "ip_adapter" not in f.read()


# ---------------------------------------------------------------------------------------------------------------- the image encoder's reader
def test_vision_state_from_both_snapshots():
    """A CLIPVisionModelWithProjection state and a whole CLIPModel state (PickScore) give the same visual.* tensors."""
    from tc_light_amd import clip
    arch = dict(embed_dim=32, image_resolution=28, vision_layers=2, vision_width=64, vision_patch_size=14, context_length=8, vocab_size=50,
                transformer_width=64, transformer_layers=1)
    sd = clip.seeded_state_dict(5, **arch)
    hf = clip.to_hf_state(sd)
    vision_only = {k: v for k, v in hf.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
    a, b = clip.from_hf_vision_state(vision_only), clip.visual_state(clip.from_hf_state(hf))
    assert set(a) == set(b) == set(clip.visual_state(sd)) and all(torch.equal(a[k], b[k]) and torch.equal(a[k], sd[k]) for k in a)
    with pytest.raises(KeyError, match="visual_projection"):
        clip.from_hf_vision_state({k: v for k, v in vision_only.items() if k != "visual_projection.weight"})
    assert clip.vision_options(None) == dict(vision_heads=16, act="gelu", crop="floor")
    flat = dict(num_attention_heads=16, hidden_act="gelu", patch_size=14, hidden_size=1280)                 # a CLIPVisionConfig: the fields at the top level
    assert clip.vision_options(flat, 1280, 14) == clip.vision_options(dict(vision_config=flat), 1280, 14) == dict(vision_heads=16, act="gelu", crop="floor")
    with pytest.raises(ValueError, match="hidden_act"):
        clip.vision_options(dict(flat, hidden_act="relu"), 1280, 14)
