"""Host side of the CLIP figures (tc_light_amd.clip, model_utils.load_clip_state, the evaluate.py decision table): no GPU."""
import os
import types

import numpy as np
import pytest
import torch

from tc_light_amd import clip as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SMALL = dict(embed_dim=64, image_resolution=64, vision_layers=2, vision_width=128, vision_patch_size=32, context_length=77, vocab_size=49408,
             transformer_width=64, transformer_layers=2)


def test_param_shapes_match_clipmodel():
    """The key set and shapes of clip_param_shapes(), through to_hf_state, are transformers.CLIPModel's at ViT-B/32 size -- and back."""
    from transformers import CLIPConfig, CLIPModel
    with torch.device("meta"):
        ref = CLIPModel(CLIPConfig()).state_dict()
    shapes = C.clip_param_shapes()
    hf = C.to_hf_state({k: torch.empty(s, device="meta") for k, s in shapes.items()})
    assert set(hf) == set(ref)
    assert all(tuple(hf[k].shape) == tuple(ref[k].shape) for k in ref), [k for k in ref if tuple(hf[k].shape) != tuple(ref[k].shape)][:3]
    back = C.from_hf_state({k: torch.empty(v.shape, device="meta") for k, v in ref.items()})
    assert {k: tuple(v.shape) for k, v in back.items()} == {k: tuple(s) for k, s in shapes.items()}


def test_hf_round_trip_is_identity():
    sd = C.seeded_state_dict(3, **SMALL)
    assert set(sd) == set(C.clip_param_shapes(**SMALL))
    back = C.from_hf_state(C.to_hf_state(sd))
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    hf = C.to_hf_state(sd)
    q = hf["text_model.encoder.layers.1.self_attn.q_proj.weight"]
    assert torch.equal(q, sd["transformer.resblocks.1.attn.in_proj_weight"][:64])
    assert torch.equal(hf["visual_projection.weight"], sd["visual.proj"].t())
    again = C.seeded_state_dict(3, **SMALL)
    assert all(torch.equal(again[k], sd[k]) for k in sd)                                  # the seed decides the weights


class _Tok:
    """The HF CLIP tokenizer interface text.py relies on: one id per word."""
    bos_token_id, eos_token_id, model_max_length = C.SOT, C.EOT, 77

    def __call__(self, txt, truncation=False, add_special_tokens=False):
        assert truncation is False and add_special_tokens is False
        return {"input_ids": [1000 + len(w) for w in txt.replace(".", " . ").split()]}


def test_tokenize_layout():
    ids = C.tokenize("soft warm light", _Tok())
    assert ids.shape == (1, 77) and ids.dtype == torch.int64
    assert ids[0, :5].tolist() == [C.SOT, 1004, 1004, 1005, C.EOT] and int(ids[0, 5:].abs().sum()) == 0
    assert int(ids.argmax(-1)) == 4                                                      # encode_text pools the EOT row
    fits = " ".join(["w"] * 75)
    assert C.tokenize(fits, _Tok())[0, 76] == C.EOT
    with pytest.raises(RuntimeError):
        C.tokenize(fits + " w", _Tok())
    with pytest.raises(FileNotFoundError):
        C.tokenize("soft light", None)
    with pytest.warns(UserWarning):
        a = C.tokenize("soft light", None, allow_random=True)
    with pytest.warns(UserWarning):
        b = C.tokenize("soft light", None, allow_random=True)
        c = C.tokenize("warm light", None, allow_random=True)
    assert torch.equal(a, b) and not torch.equal(a, c) and a[0, 0] == C.SOT and a[0, 3] == C.EOT and int(a.max()) == C.EOT


def test_long_prompt_splits_on_full_stops_and_averages(monkeypatch):
    from tc_light_amd import evaluate as E
    part = " ".join(["w"] * 40)
    prompt = f"{part}. {part} extra. "
    rows = E.prompt_id_rows(prompt, _Tok())
    assert len(rows) == 2 and int(rows[0].argmax(-1)) == 41 and int(rows[1].argmax(-1)) == 42
    assert len(E.prompt_id_rows("short. prompt", _Tok())) == 1                            # fits: not split
    monkeypatch.setattr(E, "_text_score", lambda feats, ids, engine: float(ids.argmax(-1)))
    eng = types.SimpleNamespace(context=77)
    assert E.clip_text(None, prompt, eng, _Tok(), features=torch.zeros(2, 4)) == pytest.approx(41.5)
    assert E.clip_text(None, "short. prompt", eng, _Tok(), features=torch.zeros(2, 4)) == 4.0


@pytest.mark.parametrize("H,W,want", [(720, 1280, (224, 398, 0, 87)), (1280, 720, (398, 224, 87, 0)), (224, 224, (224, 224, 0, 0)),
                                      (333, 517, (224, 347, 0, 62)), (160, 200, (224, 280, 0, 28)), (300, 225, (298, 224, 37, 0))])
def test_resize_geometry(H, W, want):
    """int(224 * long / short) and int(round((size - 224) / 2.0)): 347 - 224 = 123 -> 61.5 -> 62 (half to even)."""
    assert C.resize_geometry(H, W) == want
    short, long_ = min(H, W), max(H, W)
    assert max(want[:2]) == int(224 * long_ / short) and min(want[:2]) == 224


def test_load_clip_state_missing_file(tmp_path):
    from tc_light_amd.model_utils import load_clip_state
    with pytest.raises(FileNotFoundError):
        load_clip_state(str(tmp_path / "absent.pt"))
    with pytest.raises(FileNotFoundError):
        load_clip_state(None)
    with pytest.warns(UserWarning):
        sd = load_clip_state(str(tmp_path / "absent.pt"), allow=True)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in C.clip_param_shapes().items()}


def test_load_clip_state_reads_both_layouts(tmp_path):
    """A plain tensor file with OpenAI names and a .safetensors file with transformers names give the same state dict."""
    from safetensors.torch import save_file
    from tc_light_amd.model_utils import load_clip_state
    sd = C.seeded_state_dict(2, **SMALL)
    torch.save(sd, str(tmp_path / "clip.pt"))
    save_file({k: v.contiguous() for k, v in C.to_hf_state(sd).items()}, str(tmp_path / "model.safetensors"))
    for name in ("clip.pt", "model.safetensors"):
        got = load_clip_state(str(tmp_path / name))
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd), name


def test_evaluate_decision_table(monkeypatch):
    from tc_light_amd import evaluate as E
    monkeypatch.setenv("TCL_ALLOW_RANDOM_WEIGHTS", "1")                                   # must not switch the CLIP figures on
    assert E.NOT_COMPUTED == ("clip-frame", "clip-text", "pick-score")
    assert E.clip_settings({}) == (None, None) and E.clip_settings(None) == (None, None)
    assert E.clip_settings({"raft": "r.pth", "text_encoder": "te", "allow_random": True}) == (None, None)
    assert E.not_computed(False) == E.NOT_COMPUTED and E.not_computed(True) == ("pick-score",)
    assert E.clip_settings({"clip": "c.pt", "text_encoder": "te"}) == ("c.pt", "te")
    assert E.clip_settings({"clip": "c.pt", "text_encoder": "te", "clip_tokenizer": "ct"}) == ("c.pt", "ct")
    assert E.clip_settings({"clip": "c.pt", "clip_tokenizer": "ct"}, "cli.pt", "clitok") == ("cli.pt", "clitok")
    assert E.clip_settings({"text_encoder": "te"}, "cli.pt") == ("cli.pt", "te")
    both = E.format_results("v", "p", {"warp-error-ssim": 0.5, "clip-text": 0.25, "clip-frame": 0.987654})
    assert both == "v - p\nclip-frame: 0.9877\nclip-text: 0.2500\nwarp-error-ssim: 50.00\n"


def test_default_config_names_the_clip_paths():
    import yaml
    with open(os.path.join(ROOT, "configs", "tclight_default.yaml")) as f:
        models = yaml.safe_load(f)["models"]
    assert models["clip"].endswith("ViT-B-32.pt") and "clip_tokenizer" in models and "raft" in models


def test_symbols_declared():
    from tc_light_amd.lib import parse_header
    sig = parse_header()
    for name in ("tcl_clip_preprocess_u8", "tcl_clip_resize_geometry", "tcl_clip_attention_f16", "tcl_clip_embed_f16", "tcl_clip_quick_gelu_f16",
                 "tcl_clip_scores", "tcl_clip_scores_workspace_bytes"):
        assert name in sig, name
    src = open(os.path.join(ROOT, "tc_light_amd", "csrc", "clip.hip")).read()
    assert all(f"{name}(" in src for name in sig if name.startswith("tcl_clip_"))


def test_golden_separates_the_two_clips():
    """The golden's own guard: each figure differs between the static and the varying clip by >= 100 x the tolerance of the GPU test (4 x the floor)."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "clip.npz"))
    tol = 4 * max(float(G["f16_floor_image"]), float(G["f16_floor_text"]))
    assert abs(G["clip_frame"][0] - G["clip_frame"][1]) >= 100 * tol
    assert abs(G["clip_text"][0, 0] - G["clip_text"][0, 1]) >= 100 * tol
    assert G["frames"].dtype == np.uint8 and G["image_features"].shape == (len(G["frames"]), 512) and G["text_features"].shape == (2, 512)
