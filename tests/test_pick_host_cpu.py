"""Host side of pick-score (tc_light_amd.clip's PickScore options, tokenize_truncated, model_utils.load_pick_state, the evaluate.py decision table):
no GPU."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

from tc_light_amd import clip as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TINY = dict(embed_dim=64, image_resolution=28, vision_layers=2, vision_width=160, vision_patch_size=14, context_length=77, vocab_size=49408,
            transformer_width=128, transformer_layers=2, vision_heads=2, text_heads=2, act="gelu", eps=1e-5)


def test_pick_settings_and_decision_table(monkeypatch, tmp_path):
    from tc_light_amd import evaluate as E
    monkeypatch.setenv("TCL_ALLOW_RANDOM_WEIGHTS", "1")                                   # must not switch pick-score on
    assert E.pick_settings({}) == (None, None) and E.pick_settings(None) == (None, None)
    assert E.pick_settings({"clip": "c.pt", "text_encoder": "te", "pick": "", "pick_tokenizer": "", "allow_random": True}) == (None, None)
    assert E.pick_settings({"pick": "p", "text_encoder": "te"}) == ("p", "te")
    assert E.pick_settings({"pick": "p", "text_encoder": "te", "clip_tokenizer": "ct"}) == ("p", "ct")
    assert E.pick_settings({"pick": "p", "text_encoder": "te", "clip_tokenizer": "ct", "pick_tokenizer": "pt"}) == ("p", "pt")
    assert E.pick_settings({"pick": "p", "pick_tokenizer": "pt"}, "cli", "clitok") == ("cli", "clitok")
    assert E.pick_settings({"pick_tokenizer": "pt"}, "cli") == ("cli", "pt")
    snap = tmp_path / "snap"
    snap.mkdir()
    assert E.pick_settings({"pick": str(snap), "clip_tokenizer": "ct"}) == (str(snap), "ct")
    (snap / "vocab.json").write_text("{}")                                                # the snapshot's own vocabulary goes before the CLIP one ...
    assert E.pick_settings({"pick": str(snap), "clip_tokenizer": "ct", "text_encoder": "te"}) == (str(snap), str(snap))
    assert E.pick_settings({"pick": str(snap), "pick_tokenizer": "pt"}) == (str(snap), "pt")      # ... and after a named one
    assert E.not_computed(True, True) == () and E.not_computed(False, True) == ("clip-frame", "clip-text")
    assert E.not_computed(True, False) == ("pick-score",) and E.not_computed(False, False) == E.NOT_COMPUTED
    assert E.not_computed(False) == E.NOT_COMPUTED and E.not_computed(True) == ("pick-score",)    # the one-argument calls, as before
    four = E.format_results("v", "p", {"warp-error-ssim": 0.5, "pick-score": 21.23456, "clip-text": 0.25, "clip-frame": 0.987654})
    assert four == "v - p\nclip-frame: 0.9877\nclip-text: 0.2500\npick-score: 21.2346\nwarp-error-ssim: 50.00\n"


def test_default_config_has_empty_pick_entries():
    import yaml
    with open(os.path.join(ROOT, "configs", "tclight_default.yaml")) as f:
        models = yaml.safe_load(f)["models"]
    assert models["pick"] == "" and models["pick_tokenizer"] == "" and models["clip"].endswith("ViT-B-32.pt")


class _Tok:
    """The HF CLIP tokenizer interface: one id per word."""
    bos_token_id, eos_token_id = C.SOT, C.EOT

    def __call__(self, txt, truncation=False, add_special_tokens=False):
        assert truncation is False and add_special_tokens is False
        return {"input_ids": [1000 + i for i, _ in enumerate(txt.split())]}


def _local_vocab():
    for d in glob.glob(os.path.join(ROOT, "models", "**", "vocab.json"), recursive=True):
        if os.path.isfile(os.path.join(os.path.dirname(d), "merges.txt")):
            return os.path.dirname(d)
    return None


def test_tokenize_truncated():
    """[SOT] + ids[:75] + [EOT], unpadded: short, exactly 75 and over-long prompts.  Against CLIPTokenizer(truncation=True, max_length=77) when the
    tree holds a vocabulary, against the one-id-per-word stand-in otherwise."""
    words = {"short": 3, "fits": 75, "long": 120}
    voc = _local_vocab()
    if voc is not None:
        from transformers import CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(voc)
        for n in words.values():
            prompt = " ".join(["light"] * n)
            want = tok(prompt, padding=True, truncation=True, max_length=77)["input_ids"]
            assert C.tokenize_truncated(prompt, tok)[0].tolist() == want
    for name, n in words.items():
        ids = C.tokenize_truncated(" ".join(["w"] * n), _Tok())
        m = min(n, 75)
        assert ids.dtype == torch.int64 and ids.shape == (1, m + 2), name
        assert ids[0].tolist() == [C.SOT] + [1000 + i for i in range(m)] + [C.EOT]
        assert int(ids.argmax(-1)) == m + 1                                               # encode_text pools the EOT row
    assert C.tokenize_truncated("", _Tok())[0].tolist() == [C.SOT, C.EOT]
    assert C.tokenize_truncated("a b c d", _Tok(), context=5)[0].tolist() == [C.SOT, 1000, 1001, 1002, C.EOT]
    with pytest.raises(FileNotFoundError):
        C.tokenize_truncated("soft light", None)
    with pytest.warns(UserWarning):
        a = C.tokenize_truncated("soft light", None, allow_random=True)
        b = C.tokenize_truncated("soft light", None, allow_random=True)
        c = C.tokenize_truncated("warm light", None, allow_random=True)
        long_ = C.tokenize_truncated(" ".join(["w"] * 200), None, allow_random=True)
    assert torch.equal(a, b) and not torch.equal(a, c) and a.shape == (1, 4) and a[0, 0] == C.SOT and a[0, 3] == C.EOT
    assert long_.shape == (1, 77) and long_[0, 76] == C.EOT
    with pytest.raises(RuntimeError):                                                     # tokenize itself is unchanged: it refuses what does not fit
        C.tokenize(" ".join(["w"] * 76), _Tok())


@pytest.mark.parametrize("H,W,differ", [(227, 224, True), (224, 227, True), (448, 454, True), (720, 1280, False), (480, 853, False), (301, 224, False),
                                        (100, 60, False), (224, 224, False)])
def test_geometry_floor_vs_round(H, W, differ):
    """transformers' center_crop starts at (size - 224) // 2; clip's at int(round((size - 224) / 2.0)).  The resize is the same."""
    r, f = C.resize_geometry_rule(H, W, 224, "round"), C.resize_geometry_rule(H, W, 224, "floor")
    assert r == C.resize_geometry(H, W) and r[:2] == f[:2]
    short, long_ = min(H, W), max(H, W)
    assert (max(f[:2]), min(f[:2])) == (int(224 * long_ / short), 224)
    assert f[2:] == ((f[0] - 224) // 2, (f[1] - 224) // 2)
    assert (r != f) == differ
    if differ:
        assert sum(abs(a - b) for a, b in zip(r[2:], f[2:])) == 1
    with pytest.raises(ValueError):
        C.resize_geometry_rule(H, W, 224, "ceil")


def test_floor_geometry_is_the_transformers_processor():
    """On a 227 x 224 frame the floor rule and PIL's bicubic resize reproduce CLIPImageProcessorPil; the rounded rule is a row off."""
    from PIL import Image
    from transformers.models.clip import CLIPImageProcessorPil
    rng = np.random.default_rng(0)
    small = rng.integers(0, 256, (9, 9, 3), dtype=np.uint8)
    frame = np.asarray(Image.fromarray(small).resize((224, 227), Image.BILINEAR))
    proc = CLIPImageProcessorPil(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, resample=Image.BICUBIC)
    want = proc(images=[Image.fromarray(frame)], return_tensors="pt")["pixel_values"][0]
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(3, 1, 1)
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(3, 1, 1)
    err = {}
    for rule in ("floor", "round"):
        oh, ow, top, left = C.resize_geometry_rule(227, 224, 224, rule)
        crop = np.asarray(Image.fromarray(frame).resize((ow, oh), Image.BICUBIC))[top:top + 224, left:left + 224]
        got = (torch.from_numpy(crop.copy()).permute(2, 0, 1).float().div(255) - mean) / std
        err[rule] = float((got - want).abs().max())
    assert err["floor"] < 1e-5 and err["round"] > 1e-2, err


def test_key_mapping_on_the_hf_model():
    """from_hf_state on the full key list of transformers.CLIPModel at the PickScore configuration (1 layer per tower), with the `position_ids`
    buffers older checkpoints carry: exactly clip_param_shapes' keys and shapes."""
    from transformers import CLIPConfig, CLIPModel
    A = C.PICKSCORE_V1
    with torch.device("meta"):
        model = CLIPModel(CLIPConfig(**C.to_hf_config(A, vision_layers=1, text_layers=1)))
    vc, tc = model.config.vision_config, model.config.text_config
    assert (vc.num_attention_heads, tc.num_attention_heads, vc.hidden_act, tc.hidden_act, vc.patch_size) == (16, 16, "gelu", "gelu", 14)
    ref = dict(model.state_dict())
    ref["text_model.embeddings.position_ids"] = torch.empty(1, 77, device="meta")
    ref["vision_model.embeddings.position_ids"] = torch.empty(1, 257, device="meta")
    shapes = C.clip_param_shapes(**dict(C.arch_shapes(A), vision_layers=1, transformer_layers=1))
    back = C.from_hf_state(dict(ref))
    assert {k: tuple(v.shape) for k, v in back.items()} == {k: tuple(s) for k, s in shapes.items()}
    assert shapes["visual.conv1.weight"] == (1280, 3, 14, 14) and shapes["visual.positional_embedding"] == (257, 1280)
    left = dict(ref)
    C.from_hf_state(left, consume=True)                                                   # consuming: only the buffers are left behind
    assert sorted(left) == ["text_model.embeddings.position_ids", "vision_model.embeddings.position_ids"]
    n = sum(math.prod(s) for s in C.clip_param_shapes(**C.arch_shapes(A)).values())
    assert 985e6 < n < 987e6                                                              # the 986 M parameters of ViT-H/14 + its text tower


def test_pick_options_and_refusals():
    A = C.PICKSCORE_V1
    want = dict(vision_heads=16, text_heads=16, act="gelu", crop="floor")
    assert C.pick_options() == want
    good = C.to_hf_config(A)
    assert C.pick_options(good, 1280, 1024, 14) == want

    def cfg(tower, **kw):
        c = {k: dict(v) if isinstance(v, dict) else v for k, v in good.items()}
        c[tower].update(kw)
        return c
    for bad, field in ((cfg("vision_config", hidden_act="gelu_new"), "hidden_act"), (cfg("text_config", hidden_act="quick_gelu"), "hidden_act"),
                       (cfg("vision_config", num_attention_heads=20), None), (cfg("vision_config", num_attention_heads=32), "num_attention_heads"),
                       (cfg("text_config", num_attention_heads=8), "num_attention_heads"), (cfg("text_config", layer_norm_eps=1e-6), "layer_norm_eps"),
                       (cfg("vision_config", patch_size=16), "patch_size")):
        if field is None:                                                                 # 1280 / 20 = 64: a head_dim the kernel covers
            assert C.pick_options(bad, 1280, 1024, 14)["vision_heads"] == 20
            continue
        with pytest.raises(ValueError, match=field):
            C.pick_options(bad, 1280, 1024, 14)
    # a config.json without the fields means transformers' defaults (12 / 8 heads, quick_gelu, patch 32): refused for this checkpoint, by name
    with pytest.raises(ValueError, match="num_attention_heads"):
        C.pick_options({"vision_config": {"hidden_act": "gelu"}, "text_config": {"hidden_act": "gelu"}}, 1280, 1024, 14)
    # pick_engine refuses on the host, before any device is touched
    sd = C.seeded_state_dict(1, **C.arch_shapes(TINY))
    with pytest.raises(ValueError, match="hidden_act"):
        C.pick_engine(sd, "cuda", cfg("vision_config", hidden_act="relu"))
    with pytest.raises(ValueError, match="patch_size"):
        C.pick_engine(sd, "cuda", C.to_hf_config(dict(TINY, vision_patch_size=7)))
    with pytest.raises(KeyError):
        C.pick_engine({"logit_scale": torch.tensor(1.0)}, "cuda")
    for kw in (dict(act="relu"), dict(crop="ceil")):
        with pytest.raises(ValueError):
            C.CLIPEngine(sd, "cuda", **kw)


def test_useful_flops_at_vit_h14():
    """About 334 GFLOP per image: T = 257 tokens at width 1280 over 32 layers, whatever the head count."""
    import types
    eng = types.SimpleNamespace(vwidth=1280, grid=16, patch=14, embed_dim=1024, visual=types.SimpleNamespace(layers=[None] * 32))
    T, W = 257, 1280
    want = 2 * 256 * W * 588 + 32 * (2 * T * W * 3 * W + 4 * T * T * W + 2 * T * W * W + 16 * T * W * W) + 2 * W * 1024
    assert C.useful_flops(eng, 3) == 3 * want and 333e9 < want < 336e9


def _write_snapshot(d, sd, shards):
    from safetensors.torch import save_file
    hf = {k: v.contiguous() for k, v in C.to_hf_state(sd).items()}
    hf["text_model.embeddings.position_ids"] = torch.arange(77)[None]                     # an older checkpoint's buffer
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(C.to_hf_config(TINY), f)
    if shards == 1:
        save_file(hf, os.path.join(d, "model.safetensors"))
        return
    keys = sorted(hf)
    weight_map = {}
    for s in range(shards):
        name = f"model-{s + 1:05d}-of-{shards:05d}.safetensors"
        part = {k: hf[k] for k in keys[s::shards]}
        save_file(part, os.path.join(d, name))
        weight_map.update({k: name for k in part})
    with open(os.path.join(d, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)


def test_load_pick_state(tmp_path):
    """A sharded snapshot directory, a one-file snapshot, the bare .safetensors and a .bin all give the seeded state dict back, with the config
    where there is one; a shard that its index names but the directory lacks is an error."""
    from tc_light_amd.model_utils import load_pick_state
    sd = C.seeded_state_dict(2, **C.arch_shapes(TINY))
    _write_snapshot(str(tmp_path / "sharded"), sd, 3)
    _write_snapshot(str(tmp_path / "single"), sd, 1)
    torch.save({k: v.contiguous() for k, v in C.to_hf_state(sd).items()}, str(tmp_path / "pytorch_model.bin"))
    for path, has_config in ((tmp_path / "sharded", True), (tmp_path / "single", True), (tmp_path / "single" / "model.safetensors", False),
                             (tmp_path / "pytorch_model.bin", False)):
        got, config = load_pick_state(str(path))
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) and got[k].dtype == sd[k].dtype for k in sd), path
        assert (config == C.to_hf_config(TINY)) if has_config else config is None
        if has_config:
            assert C.pick_options(config, 160, 128, 14) == dict(vision_heads=2, text_heads=2, act="gelu", crop="floor")
    os.remove(str(tmp_path / "sharded" / "model-00002-of-00003.safetensors"))
    with pytest.raises(FileNotFoundError, match="model-00002-of-00003"):
        load_pick_state(str(tmp_path / "sharded"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError):
        load_pick_state(str(tmp_path / "empty"))


def test_load_pick_state_missing_path(tmp_path, monkeypatch):
    """A missing path is an error; with allow it is the seeded PICKSCORE_V1 stand-in (the generator is replaced here: 986 M normals take a while)."""
    from tc_light_amd import model_utils as M
    with pytest.raises(FileNotFoundError):
        M.load_pick_state(str(tmp_path / "absent"))
    with pytest.raises(FileNotFoundError):
        M.load_pick_state(None)
    seen = {}
    monkeypatch.setattr(C, "seeded_state_dict", lambda seed, **arch: seen.update(seed=seed, arch=arch) or {"stand-in": True})
    with pytest.warns(UserWarning):
        sd, config = M.load_pick_state(str(tmp_path / "absent"), allow=True)
    assert sd == {"stand-in": True} and config is None
    assert seen["arch"] == C.arch_shapes(C.PICKSCORE_V1) and seen["arch"]["vision_patch_size"] == 14 and len(seen["arch"]) == 9


def test_symbols_declared():
    from tc_light_amd.lib import parse_header
    sig = parse_header()
    for name in ("tcl_clip_preprocess_ld_u8", "tcl_clip_resize_geometry_rule", "tcl_pick_scores"):
        assert name in sig, name
    src = open(os.path.join(ROOT, "tc_light_amd", "csrc", "clip.hip")).read()
    assert all(f"{name}(" in src for name in sig if name.startswith("tcl_pick_"))


def test_golden_separates_the_two_clips():
    """The golden's own guard: the two clips' pick-scores differ by >= 10 x the GPU test's tolerance exp(logit_scale) (2 floor_image + 2 floor_text);
    it holds frames at a size where the two crop rules differ, a prompt that is truncated, and no weights."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "pick.npz"))
    tol = math.exp(float(G["logit_scale"])) * (2 * float(G["f16_floor_image"]) + 2 * float(G["f16_floor_text"]))
    assert abs(G["pick_score"][0, 0] - G["pick_score"][0, 1]) >= 10 * tol
    assert G["frames_a"].dtype == np.uint8 and G["frames_a"].shape[1:] == (227, 224, 3)
    assert C.resize_geometry_rule(227, 224, 224, "floor") != C.resize_geometry_rule(227, 224, 224, "round")
    n = len(G["frames_a"]) + len(G["frames_b"])
    assert G["image_features"].shape == (n, 1024) and G["text_features"].shape == (2, 1024) and G["scores"].shape == (2, n)
    assert len(G["raw_ids_1"]) > 75 and len(G["raw_ids_0"]) < 75
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pick.npz")) < 1 << 20
    na = len(G["frames_a"])
    assert np.allclose(G["pick_score"][:, 0], G["scores"][:, :na].mean(1)) and np.allclose(G["pick_score"][:, 1], G["scores"][:, na:].mean(1))
