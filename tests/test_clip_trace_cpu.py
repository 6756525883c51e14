"""CPU: what the CLIP engines send to the device, and the seeded weights they are tested on.  tc_light_amd.clip's `lib()` becomes a recorder that
notes every launch as (name, *the arguments that are not tensors: sizes, strides, flags, eps, a 0 for an absent pointer, the stream) and its
`stream()` 0, so both engines run on device "cpu" (their outputs are then uninitialised memory; only the launches are looked at).  The expected
lists and digests below were recorded before the host path was restructured (one text tower, one name map) and are never computed from the code
under test: names, order and every scalar have to come out the same."""
import hashlib

import pytest
import torch

from tc_light_amd import clip as C

TINY = dict(embed_dim=64, image_resolution=28, vision_layers=1, vision_width=128, vision_patch_size=14, context_length=8, vocab_size=50,
            transformer_width=64, transformer_layers=2)
TINY_TEXT = dict(width=64, layers=1, context_length=8, vocab_size=50)

# CLIPEngine(TINY, vision_heads=2, text_heads=1, act="gelu", crop="floor").encode_image(three 30 x 40 frames, batch=2): batches of 2 and 1
GELU_IMAGE = [
    ('tcl_clip_preprocess_ld_u8', 0, 2, 30, 40, 28, 14, 640, 1, 0),
    ('tcl_gemm_f16', 0, 0, 8, 128, 640, 640, 640, 128, 128, 0, 0),
    ('tcl_clip_embed_f16', 0, 0, 2, 5, 128, 0, 1e-05, 0),
    ('tcl_layernorm_f16', 10, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 10, 384, 128, 128, 128, 384, 384, 0, 0),
    ('tcl_clip_attention_f16', 2, 5, 2, 64, 0.125, 0, 0),
    ('tcl_gemm_f16', 10, 128, 128, 128, 128, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 10, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 10, 512, 128, 128, 128, 512, 512, 4, 0),
    ('tcl_gemm_f16', 10, 128, 512, 512, 512, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 2, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 0, 2, 64, 128, 128, 128, 64, 64, 0, 0),
    ('tcl_clip_preprocess_ld_u8', 0, 1, 30, 40, 28, 14, 640, 1, 0),
    ('tcl_gemm_f16', 0, 0, 4, 128, 640, 640, 640, 128, 128, 0, 0),
    ('tcl_clip_embed_f16', 0, 0, 1, 5, 128, 0, 1e-05, 0),
    ('tcl_layernorm_f16', 5, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 384, 128, 128, 128, 384, 384, 0, 0),
    ('tcl_clip_attention_f16', 1, 5, 2, 64, 0.125, 0, 0),
    ('tcl_gemm_f16', 5, 128, 128, 128, 128, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 5, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 512, 128, 128, 128, 512, 512, 4, 0),
    ('tcl_gemm_f16', 5, 128, 512, 512, 512, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 1, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 0, 1, 64, 128, 128, 128, 64, 64, 0, 0),
]
# the same engine's encode_text([[48, 3, 4, 49, 0]]): two causal blocks, ln_final on the end-of-text row, the projection
GELU_TEXT = [
    ('tcl_clip_embed_f16', 0, 0, 0, 0, 1, 5, 64, 50, 1e-05, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 192, 64, 64, 64, 192, 192, 0, 0),
    ('tcl_clip_attention_f16', 1, 5, 1, 64, 0.125, 1, 0),
    ('tcl_gemm_f16', 5, 64, 64, 64, 64, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 256, 64, 64, 64, 256, 256, 4, 0),
    ('tcl_gemm_f16', 5, 64, 256, 256, 256, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 192, 64, 64, 64, 192, 192, 0, 0),
    ('tcl_clip_attention_f16', 1, 5, 1, 64, 0.125, 1, 0),
    ('tcl_gemm_f16', 5, 64, 64, 64, 64, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 256, 64, 64, 64, 256, 256, 4, 0),
    ('tcl_gemm_f16', 5, 64, 256, 256, 256, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 1, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 0, 1, 64, 64, 64, 64, 64, 64, 0, 0),
]
# CLIPTextEngine(TINY_TEXT, heads=1).hidden_states([[48, 3, 49]]): one QuickGELU block, ln_final on every row
HIDDEN = [
    ('tcl_clip_embed_f16', 0, 0, 0, 0, 1, 3, 64, 50, 1e-05, 0),
    ('tcl_layernorm_f16', 3, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 3, 192, 64, 64, 64, 192, 192, 0, 0),
    ('tcl_clip_attention_f16', 1, 3, 1, 64, 0.125, 1, 0),
    ('tcl_gemm_f16', 3, 64, 64, 64, 64, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 3, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 3, 256, 64, 64, 64, 256, 256, 0, 0),
    ('tcl_clip_quick_gelu_f16', 768, 0),
    ('tcl_gemm_f16', 3, 64, 256, 256, 256, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 3, 64, 1e-05, 0),
]
# CLIPEngine with its defaults (QuickGELU, rounded crop) at patch 32 / resolution 64: tcl_clip_preprocess_u8 and the QuickGELU pass
QUICK_IMAGE = [
    ('tcl_clip_preprocess_u8', 0, 2, 30, 40, 64, 32, 0),
    ('tcl_gemm_f16', 0, 0, 8, 128, 3072, 3072, 3072, 128, 128, 0, 0),
    ('tcl_clip_embed_f16', 0, 0, 2, 5, 128, 0, 1e-05, 0),
    ('tcl_layernorm_f16', 10, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 10, 384, 128, 128, 128, 384, 384, 0, 0),
    ('tcl_clip_attention_f16', 2, 5, 2, 64, 0.125, 0, 0),
    ('tcl_gemm_f16', 10, 128, 128, 128, 128, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 10, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 10, 512, 128, 128, 128, 512, 512, 0, 0),
    ('tcl_clip_quick_gelu_f16', 5120, 0),
    ('tcl_gemm_f16', 10, 128, 512, 512, 512, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 2, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 0, 2, 64, 128, 128, 128, 64, 64, 0, 0),
    ('tcl_clip_preprocess_u8', 0, 1, 30, 40, 64, 32, 0),
    ('tcl_gemm_f16', 0, 0, 4, 128, 3072, 3072, 3072, 128, 128, 0, 0),
    ('tcl_clip_embed_f16', 0, 0, 1, 5, 128, 0, 1e-05, 0),
    ('tcl_layernorm_f16', 5, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 384, 128, 128, 128, 384, 384, 0, 0),
    ('tcl_clip_attention_f16', 1, 5, 2, 64, 0.125, 0, 0),
    ('tcl_gemm_f16', 5, 128, 128, 128, 128, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 5, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 512, 128, 128, 128, 512, 512, 0, 0),
    ('tcl_clip_quick_gelu_f16', 2560, 0),
    ('tcl_gemm_f16', 5, 128, 512, 512, 512, 128, 128, 0, 0),
    ('tcl_layernorm_f16', 1, 128, 1e-05, 0),
    ('tcl_gemm_f16', 0, 0, 1, 64, 128, 128, 128, 64, 64, 0, 0),
]
QUICK_TEXT = [
    ('tcl_clip_embed_f16', 0, 0, 0, 0, 1, 5, 64, 50, 1e-05, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 192, 64, 64, 64, 192, 192, 0, 0),
    ('tcl_clip_attention_f16', 1, 5, 1, 64, 0.125, 1, 0),
    ('tcl_gemm_f16', 5, 64, 64, 64, 64, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 256, 64, 64, 64, 256, 256, 0, 0),
    ('tcl_clip_quick_gelu_f16', 1280, 0),
    ('tcl_gemm_f16', 5, 64, 256, 256, 256, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 192, 64, 64, 64, 192, 192, 0, 0),
    ('tcl_clip_attention_f16', 1, 5, 1, 64, 0.125, 1, 0),
    ('tcl_gemm_f16', 5, 64, 64, 64, 64, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 5, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 5, 256, 64, 64, 64, 256, 256, 0, 0),
    ('tcl_clip_quick_gelu_f16', 1280, 0),
    ('tcl_gemm_f16', 5, 64, 256, 256, 256, 64, 64, 0, 0),
    ('tcl_layernorm_f16', 1, 64, 1e-05, 0),
    ('tcl_gemm_f16', 0, 0, 1, 64, 64, 64, 64, 64, 64, 0, 0),
]


class _Recorder:
    def __init__(self):
        self.trace = []

    def __getattr__(self, name):
        def launch(*args):
            self.trace.append((name,) + tuple(a for a in args if not torch.is_tensor(a)))
            return 0
        return launch


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(C, "lib", lambda: r)
    monkeypatch.setattr(C, "stream", lambda: 0)
    return r


def _frames(n=3, H=30, W=40):
    return torch.arange(n * H * W * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(n, H, W, 3)


def test_launch_trace(rec):
    """CLIPEngine (erf GELU, floored crop, padded patch rows: the PickScore branches), CLIPTextEngine, and CLIPEngine with OpenAI's defaults
    (QuickGELU, tcl_clip_preprocess_u8): the same launches in the same order with the same scalars as before the restructuring."""
    eng = C.CLIPEngine(C.seeded_state_dict(3, **TINY), "cpu", vision_heads=2, text_heads=1, act="gelu", crop="floor")
    feats = eng.encode_image(_frames(), batch=2)
    assert feats.shape == (3, 64) and feats.dtype == torch.float32
    n_image = len(rec.trace)
    assert eng.encode_text([[48, 3, 4, 49, 0]]).shape == (1, 64)
    n_text = len(rec.trace)
    txt = C.CLIPTextEngine(C.seeded_text_state_dict(4, **TINY_TEXT), "cpu", heads=1)
    out = txt.hidden_states([[48, 3, 49]])
    assert out.shape == (1, 3, 64) and out.dtype == torch.float16
    assert len(rec.trace) == 51
    assert rec.trace[:n_image] == GELU_IMAGE
    assert rec.trace[n_image:n_text] == GELU_TEXT
    assert rec.trace[n_text:] == HIDDEN
    del rec.trace[:]
    quick = C.CLIPEngine(C.seeded_state_dict(3, **dict(TINY, image_resolution=64, vision_patch_size=32)), "cpu")
    quick.encode_image(_frames(), batch=2)
    n_image = len(rec.trace)
    quick.encode_text([[48, 3, 4, 49, 0]])
    assert rec.trace[:n_image] == QUICK_IMAGE
    assert rec.trace[n_image:] == QUICK_TEXT


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.contiguous().numpy().tobytes())
    return h.hexdigest()


def test_seeded_weights_are_pinned():
    """Key order and draw order of the two seeded state dicts: the goldens were made from these draws."""
    assert _digest(C.seeded_state_dict(3, **TINY)) == "fc883db0e3635d96ca459a26c4aa1a39d9da90e02d32991f29a5e8bacf330158"
    assert _digest(C.seeded_text_state_dict(4, **TINY_TEXT)) == "642948b06a5fb8b7ad95ea9c2fca65855b43148124e05b3846f047383633cf5e"
