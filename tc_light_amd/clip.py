"""OpenAI CLIP on the device: the model behind the clip-frame and clip-text figures of the reference's evaluate.py (evaluate.py:119
`clip.load("ViT-B/32")`; utils/evaluation/eval_utils.py:129-161).

`CLIPEngine` = clip/model.py's CLIP in inference: `encode_image` is `preprocess` (Resize(BICUBIC) -> CenterCrop -> ToTensor -> Normalize, one kernel on
the uint8 frames) -> conv1 as a GEMM over patch rows -> [class | patches] + positional embedding -> ln_pre -> the pre-LN residual blocks -> ln_post on
the class token -> proj; `encode_text` is token + positional embedding -> the same blocks with the causal mask -> ln_final on the row of the
end-of-text token (`ids.argmax(-1)`) -> text_projection.  A block is LayerNorm, the fused in_proj GEMM, tcl_clip_attention_f16 (which reads the GEMM's
[q | k | v] rows in place), out_proj with the residual in its epilogue, LayerNorm, c_fc, QuickGELU, c_proj with the residual.  Widths, depth, patch
size and context length come from the tensor shapes and the head count is width // 64 (clip/model.py build_model), so another CLIP of this family
loads unchanged.  Activations are f16 with f32 accumulation; the features are returned as f32.

The same engine runs PickScore_v1, the model behind pick-score (evaluate.py:52-56,120-121; eval_utils.py:163-176): a transformers.CLIPModel at CLIP
ViT-H/14 (`PICKSCORE_V1`), built by `pick_engine` with what its tensors do not say: 16 heads per tower, erf GELU (c_fc's GEMM epilogue), and the
preprocessing of transformers' image processor, whose centre crop is floored where clip's is rounded.  A patch size whose 3 P^2 is not a multiple of
64 (14: 588) gets patch rows and a conv1 weight zero-padded to the next multiple.  `tokenize_truncated` is that processor's text side and
`pick_scores` the figure (tcl_pick_scores).  Pinned by tests/golden/pick.npz (tests/test_gpu_pick.py).

State dicts use OpenAI's key names.  `from_hf_state` / `to_hf_state` map to and from `transformers.CLIPModel`'s names (q / k / v concatenated into
in_proj, the projections transposed).  Pinned against `transformers.CLIPModel` in f32 by tests/golden/clip.npz (tests/test_gpu_clip.py).

`CLIPTextEngine` is the text tower alone, read at every position (ln_final on all rows, no projection): `transformers.CLIPTextModel`'s
last_hidden_state, the prompt embeddings of SD-1.5 (`SD15_TEXT`, the text tower of CLIP ViT-L/14; tc_light_amd/text.py).  `from_hf_text_state` /
`to_hf_text_state` map a text_encoder checkpoint, `text_options` reads its config.json.  Pinned by tests/golden/text.npz (tests/test_gpu_text.py).

Structure: `_tower_to_hf` / `_tower_from_hf` are the per-layer renaming, one per direction, under the four state-dict maps; `_prompt_ids` is the
tokenizer front of `tokenize` and `tokenize_truncated`; `_check_tower` holds the rules on heads, activation and eps for `_Tower`, `pick_options` and
`text_options`.  `_Blocks` is the launches of a block sequence, built from (device, act, eps).  `_TextTower` is a `_Blocks` with the token table,
positional rows, ln_final and the text `_Tower`: CLIPTextEngine is one plus `hidden_states`.  `_ImageTower` is a `_Blocks` with the image side
(`encode_image`): CLIPVisionEngine is one alone (IP-Adapter's image encoder); CLIPEngine is one that also holds a `_TextTower` for `encode_text`.  tests/test_clip_trace_cpu.py pins the launches of both.
"""
import hashlib
import math
import warnings

import numpy as np
import torch

from .lib import lib, stream

H16 = torch.float16
HEAD_DIM = 64                                                            # clip/model.py build_model: heads = width // 64
VIT_B32 = dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32, context_length=77, vocab_size=49408,
               transformer_width=512, transformer_layers=12)
SOT, EOT = 49406, 49407                                                  # <|startoftext|>, <|endoftext|> of clip's BPE vocabulary
# pickapic-anonymous/PickScore_v1 (evaluate.py:120-121): transformers.CLIPModel at CLIP ViT-H/14 (laion/CLIP-ViT-H-14-laion2B-s32B-b79K).  The first
# nine entries are clip_param_shapes' arguments (arch_shapes); the rest is what a transformers checkpoint keeps in config.json, not in its tensors.
PICKSCORE_V1 = dict(embed_dim=1024, image_resolution=224, vision_layers=32, vision_width=1280, vision_patch_size=14, context_length=77,
                    vocab_size=49408, transformer_width=1024, transformer_layers=24, vision_heads=16, text_heads=16, act="gelu", eps=1e-5)
# SD-1.5's text_encoder: the text tower of CLIP ViT-L/14, read at last_hidden_state (CLIPTextEngine; text_param_shapes takes the first four entries)
SD15_TEXT = dict(width=768, layers=12, context_length=77, vocab_size=49408, heads=12, act="quick_gelu", eps=1e-5)
ACTS = {"quick_gelu": 0, "gelu": 4}                                     # -> tcl_gemm_f16's act of c_fc (QuickGELU is a pass of its own)
CROPS = {"round": 0, "floor": 1}                                         # -> the crop rule of tcl_clip_preprocess_ld_u8


# ---- state dicts
def _block_shapes(sh, prefix, width):
    sh[prefix + "attn.in_proj_weight"] = (3 * width, width); sh[prefix + "attn.in_proj_bias"] = (3 * width,)
    sh[prefix + "attn.out_proj.weight"] = (width, width); sh[prefix + "attn.out_proj.bias"] = (width,)
    sh[prefix + "ln_1.weight"] = (width,); sh[prefix + "ln_1.bias"] = (width,)
    sh[prefix + "mlp.c_fc.weight"] = (4 * width, width); sh[prefix + "mlp.c_fc.bias"] = (4 * width,)
    sh[prefix + "mlp.c_proj.weight"] = (width, 4 * width); sh[prefix + "mlp.c_proj.bias"] = (width,)
    sh[prefix + "ln_2.weight"] = (width,); sh[prefix + "ln_2.bias"] = (width,)
    return sh


_BLOCK_KEYS = tuple(_block_shapes({}, "", 0))                           # the twelve tensors of a block, as _Tower loads them


def text_param_shapes(width=768, layers=12, context_length=77, vocab_size=49408):
    """State-dict keys and shapes of a text tower alone, as CLIPTextEngine takes it (the defaults are SD15_TEXT): no text_projection, no visual.*."""
    sh = {"token_embedding.weight": (vocab_size, width), "positional_embedding": (context_length, width)}
    for i in range(layers):
        _block_shapes(sh, f"transformer.resblocks.{i}.", width)
    sh["ln_final.weight"] = (width,); sh["ln_final.bias"] = (width,)
    return sh


def clip_param_shapes(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32, context_length=77,
                      vocab_size=49408, transformer_width=512, transformer_layers=12):
    """State-dict keys and shapes of clip/model.py's CLIP with a VisionTransformer tower (the defaults are ViT-B/32).  The key order is the order
    `_seeded` draws in, which the goldens were made from: the image tower, text_param_shapes' keys in their order, the two text-side scalars."""
    sh = {}
    vw = vision_width
    grid = image_resolution // vision_patch_size
    sh["visual.class_embedding"] = (vw,)
    sh["visual.positional_embedding"] = (grid * grid + 1, vw)
    sh["visual.conv1.weight"] = (vw, 3, vision_patch_size, vision_patch_size)
    sh["visual.ln_pre.weight"] = (vw,); sh["visual.ln_pre.bias"] = (vw,)
    for i in range(vision_layers):
        _block_shapes(sh, f"visual.transformer.resblocks.{i}.", vw)
    sh["visual.ln_post.weight"] = (vw,); sh["visual.ln_post.bias"] = (vw,)
    sh["visual.proj"] = (vw, embed_dim)
    sh.update(text_param_shapes(transformer_width, transformer_layers, context_length, vocab_size))
    sh["text_projection"] = (transformer_width, embed_dim)
    sh["logit_scale"] = ()
    return sh


def arch_shapes(arch):
    """The entries of an architecture dictionary (VIT_B32, PICKSCORE_V1) that clip_param_shapes / seeded_state_dict take."""
    return {k: arch[k] for k in VIT_B32 if k in arch}


def _seeded(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes.items():
        if k == "logit_scale":
            sd[k] = torch.tensor(math.log(1 / 0.07))
            continue
        r = torch.randn(*s, generator=g)
        if k.endswith("in_proj_weight"):
            v = r * (1.0 / math.sqrt(s[1]))
        elif k.endswith("out_proj.weight") or k.endswith("c_proj.weight"):
            v = r * (0.7 / math.sqrt(s[1]))
        elif k.endswith("c_fc.weight"):
            v = r / math.sqrt(s[1])
        elif k.endswith("conv1.weight"):
            v = r / math.sqrt(s[1] * s[2] * s[3])
        elif k in ("visual.proj", "text_projection"):
            v = r * (0.75 ** torch.arange(s[1], dtype=torch.float32).clamp(max=40))[None] / math.sqrt(s[0])
        elif k.endswith("ln_1.weight") or k.endswith("ln_2.weight") or k in ("visual.ln_pre.weight", "visual.ln_post.weight", "ln_final.weight"):
            v = 1.0 + 0.1 * r
        elif k.endswith("bias"):
            v = 0.1 * r
        elif k in ("visual.class_embedding", "visual.positional_embedding", "positional_embedding"):
            v = 0.3 * r
        else:                                                           # token_embedding
            v = r
        sd[k] = v.contiguous()
    return sd


def seeded_state_dict(seed=6, **arch):
    """Seeded stand-in weights of the architecture (default ViT-B/32), scaled so that the features depend on the input -- with the usual small
    initialisation the class token barely hears the patches and every image gets almost the same feature.  Linears are N(0, g^2 / fan_in) with
    g = 1 for in_proj (attention logits of about one unit: the softmax selects) and the MLP's c_fc, and 0.7 for the two output projections of a
    block; LayerNorm weights 1 +- 0.1, biases +- 0.1; embeddings N(0, 1) (class / positional at 0.3); the columns of the two final projections
    decay as 0.75^j, so a feature lives mostly in a few directions and cosines between features of unrelated inputs spread over [-1, 1]."""
    return _seeded(clip_param_shapes(**arch), seed)


def seeded_text_state_dict(seed=8, **arch):
    """seeded_state_dict's recipe on the keys of text_param_shapes.  `arch` is an architecture dictionary such as SD15_TEXT; the entries that are not
    shapes (heads, act, eps) are CLIPTextEngine's business and are ignored here."""
    return _seeded(text_param_shapes(**{k: v for k, v in arch.items() if k in ("width", "layers", "context_length", "vocab_size")}), seed)


_HF_BLOCK = (("ln_1.", "layer_norm1."), ("ln_2.", "layer_norm2."), ("attn.out_proj.", "self_attn.out_proj."), ("mlp.c_fc.", "mlp.fc1."),
             ("mlp.c_proj.", "mlp.fc2."))
_HF_TOP = (("visual.class_embedding", "vision_model.embeddings.class_embedding"),
           ("visual.positional_embedding", "vision_model.embeddings.position_embedding.weight"),
           ("visual.conv1.weight", "vision_model.embeddings.patch_embedding.weight"),
           ("visual.ln_pre.weight", "vision_model.pre_layrnorm.weight"), ("visual.ln_pre.bias", "vision_model.pre_layrnorm.bias"),
           ("visual.ln_post.weight", "vision_model.post_layernorm.weight"), ("visual.ln_post.bias", "vision_model.post_layernorm.bias"),
           ("token_embedding.weight", "text_model.embeddings.token_embedding.weight"),
           ("positional_embedding", "text_model.embeddings.position_embedding.weight"),
           ("ln_final.weight", "text_model.final_layer_norm.weight"), ("ln_final.bias", "text_model.final_layer_norm.bias"),
           ("logit_scale", "logit_scale"))
_HF_TOWERS = (("visual.transformer.resblocks.", "vision_model.encoder.layers."), ("transformer.resblocks.", "text_model.encoder.layers."))


def _layers(sd, prefix):
    return 1 + max(int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix))


def _tower_to_hf(out, take, n, oa, hf):
    """n layers of a tower into `out`: OpenAI names under `oa`, read through `take` -> transformers names under `hf`; in_proj split into q / k / v."""
    for i in range(n):
        a, h = f"{oa}{i}.", f"{hf}{i}."
        for kind in ("weight", "bias"):
            for name, part in zip("qkv", take(a + "attn.in_proj_" + kind).chunk(3, 0)):
                out[h + f"self_attn.{name}_proj." + kind] = part.contiguous()
            for x, y in _HF_BLOCK:
                out[h + y + kind] = take(a + x + kind)


def _tower_from_hf(out, take, n, oa, hf):
    """The inverse of _tower_to_hf: transformers names under `hf`, read through `take` -> OpenAI names under `oa`; q / k / v copied into in_proj."""
    for i in range(n):
        a, h = f"{oa}{i}.", f"{hf}{i}."
        for kind in ("weight", "bias"):
            out[a + "attn.in_proj_" + kind] = torch.cat([take(h + f"self_attn.{name}_proj." + kind) for name in "qkv"]).contiguous()
            for x, y in _HF_BLOCK:
                out[a + x + kind] = take(h + y + kind)


def to_hf_state(sd):
    """OpenAI names -> `transformers.CLIPModel` names: in_proj split into q / k / v, `visual.proj` / `text_projection` transposed into Linear weights."""
    out = {hf: sd[oa] for oa, hf in _HF_TOP}
    out["visual_projection.weight"] = sd["visual.proj"].t().contiguous()
    out["text_projection.weight"] = sd["text_projection"].t().contiguous()
    for oa, hf in _HF_TOWERS:
        _tower_to_hf(out, sd.__getitem__, _layers(sd, oa), oa, hf)
    return out


def from_hf_state(sd, consume=False):
    """`transformers.CLIPModel` names -> OpenAI names (the inverse of to_hf_state; `position_ids` buffers of older checkpoints are dropped).
    consume: entries are removed from `sd` as they are used, so a large checkpoint is never held twice (q / k / v are copied into in_proj)."""
    take = sd.pop if consume else sd.__getitem__
    out = {oa: take(hf) for oa, hf in _HF_TOP}
    out["visual.proj"] = take("visual_projection.weight").t().contiguous()
    out["text_projection"] = take("text_projection.weight").t().contiguous()
    for oa, hf in _HF_TOWERS:
        _tower_from_hf(out, take, _layers(sd, hf), oa, hf)
    return out


_HF_TEXT = "text_model."
_HF_TEXT_TOP = tuple((oa, hf) for oa, hf in _HF_TOP if hf.startswith(_HF_TEXT))


def with_text_prefix(sd):
    """A `transformers.CLIPTextModel` state dict in the `text_model.`-prefixed spelling: checkpoints on disk carry the prefix, the state dict of a
    recent transformers' CLIPTextModel does not.  The LoRA names of the text encoder (lora_te_text_model_...) are derived from the prefixed form."""
    return {(k if k.startswith(_HF_TEXT) else _HF_TEXT + k): v for k, v in sd.items()}


def to_hf_text_state(sd, prefix=_HF_TEXT):
    """OpenAI names of a text tower -> `transformers.CLIPTextModel` names (in_proj split into q / k / v), under `prefix` ("text_model." as in the
    checkpoints, or "" for a transformers whose CLIPTextModel has no such level)."""
    out = {prefix + hf[len(_HF_TEXT):]: sd[oa] for oa, hf in _HF_TEXT_TOP}
    oa, hf = _HF_TOWERS[1]
    _tower_to_hf(out, sd.__getitem__, _layers(sd, oa), oa, prefix + hf[len(_HF_TEXT):])
    return out


def from_hf_text_state(sd):
    """`transformers.CLIPTextModel` names, with or without the leading `text_model.` -> OpenAI names (the inverse of to_hf_text_state).  The
    `embeddings.position_ids` buffer of older checkpoints is ignored, as is any other key the tower does not have."""
    sd = with_text_prefix(sd)
    missing = [hf for _, hf in _HF_TEXT_TOP if hf not in sd]
    if missing:
        raise KeyError(f"text encoder state dict lacks {missing[:3]} (transformers.CLIPTextModel's key names)")
    out = {oa: sd[hf] for oa, hf in _HF_TEXT_TOP}
    oa, hf = _HF_TOWERS[1]
    _tower_from_hf(out, sd.__getitem__, _layers(sd, hf), oa, hf)
    return out


# ---- geometry and tokens
def resize_geometry_rule(H, W, side=224, crop="round"):
    """The sizes of the preprocessing for an H x W frame -> (resized height, resized width, crop top, crop left).  Resize puts the short side at
    `side` and the long one at int(side * long / short).  The crop rule is named: "round" is clip's CenterCrop, which starts at
    int(round((size - side) / 2.0)); "floor" is transformers' `center_crop` (image_transforms.py: top = (size - side) // 2), the rule of the
    processor PickScore is fed by.  The two differ by one row or column when size - side is 2 (mod 4), e.g. 227 -> 224.
    (tcl_clip_resize_geometry_rule is the same on the C side.)"""
    if crop not in CROPS:
        raise ValueError(f"crop must be one of {sorted(CROPS)}, got {crop!r}")
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(side * long_ / short)
    oh, ow = (new_long, side) if W <= H else (side, new_long)
    if crop == "floor":
        return oh, ow, (oh - side) // 2, (ow - side) // 2
    return oh, ow, int(round((oh - side) / 2.0)), int(round((ow - side) / 2.0))


def resize_geometry(H, W, side=224):
    """The sizes of clip's `_transform(side)`: resize_geometry_rule with the rounded crop (as tcl_clip_resize_geometry on the C side)."""
    return resize_geometry_rule(H, W, side, "round")


def _prompt_ids(prompt, tokenizer, allow_random, setting):
    """-> (the prompt's ids, the start id, the end id) from any tokenizer with the HF CLIP interface (`tokenizer(txt, truncation=False,
    add_special_tokens=False)["input_ids"]`, `.bos_token_id`, `.eos_token_id`).  tokenizer None: an error naming `setting`, the caller's configuration
    entry, unless `allow_random`, which gives a deterministic text-seeded id sequence (one id per word) with a warning."""
    if tokenizer is not None:
        return list(tokenizer(prompt, truncation=False, add_special_tokens=False)["input_ids"]), int(tokenizer.bos_token_id), int(tokenizer.eos_token_id)
    if not allow_random:
        raise FileNotFoundError(f"no CLIP tokenizer (models.{setting} / --{setting}); set models.allow_random / "
                                "TCL_ALLOW_RANDOM_WEIGHTS=1 for deterministic stand-in token ids")
    warnings.warn("CLIP tokenizer not found -> deterministic text-seeded stand-in token ids (allow_random)")
    seed = int.from_bytes(hashlib.sha256(prompt.encode()).digest()[:4], "little")
    n = max(1, len(prompt.replace(",", " , ").replace(".", " . ").split()))
    return np.random.default_rng(seed).integers(1000, 40000, n).tolist(), SOT, EOT


def tokenize(prompt, tokenizer, context=77, allow_random=False):
    """clip.tokenize([prompt]): int64 [1, context] = [SOT] + ids + [EOT], zero-padded.  RuntimeError when the prompt does not fit, as clip.tokenize
    raises (the caller then splits on '.', evaluate.py:43-49).  `tokenizer` and `allow_random`: see _prompt_ids."""
    ids, sot, eot = _prompt_ids(prompt, tokenizer, allow_random, "clip_tokenizer")
    if len(ids) + 2 > context:
        raise RuntimeError(f"Input {prompt!r} is too long for context length {context}")
    out = torch.zeros(1, context, dtype=torch.int64)
    out[0, :len(ids) + 2] = torch.tensor([sot] + ids + [eot], dtype=torch.int64)
    return out


def tokenize_truncated(prompt, tokenizer, context=77, allow_random=False):
    """`processor(text=prompt, padding=True, truncation=True, max_length=context)` on one prompt (eval_utils.py:163-176 pick_score_func): int64
    [1, n + 2] = [SOT] + ids[:context - 2] + [EOT], unpadded (one prompt is its own longest) and truncated, so nothing is "too long".  `tokenizer`
    and `allow_random`: see _prompt_ids."""
    ids, sot, eot = _prompt_ids(prompt, tokenizer, allow_random, "pick_tokenizer")
    return torch.tensor([[sot] + ids[:max(0, context - 2)] + [eot]], dtype=torch.int64)


def load_tokenizer(tok_dir):
    """CLIP's tokenizer (bpe.CLIPBPE) from a local directory (the directory itself or its `tokenizer` sub-directory: vocab.json + merges.txt), or None
    when there is none."""
    from .bpe import CLIPBPE
    return CLIPBPE.from_dir(tok_dir) if tok_dir else None


# ---- the engine
HEAD_DIMS = tuple(range(16, 129, 16))                                    # what tcl_clip_attention_f16 takes
_HF_FIELDS = ("num_attention_heads", "hidden_act", "layer_norm_eps")     # a transformers config.json's names for heads, act, eps


def _check_tower(width, heads, act, eps=1e-5, head_dims=HEAD_DIMS, fields=("heads", "act", "eps"), where=""):
    """What the kernels cover in one tower: a head count that divides the width into a head_dim of `head_dims`, an activation of ACTS, LayerNorms
    at the eps they are tested at.  ValueError naming the field as the caller's source spells it (`fields`; `where` says which tower)."""
    if not isinstance(heads, int) or heads <= 0 or width % heads or width // heads not in head_dims:
        raise ValueError(f"{fields[0]}{where}: {heads!r} heads on width {width}; head_dim must be one of {list(head_dims)} (tcl_clip_attention_f16)")
    if act not in ACTS:
        raise ValueError(f"{fields[1]}{where}: {act!r}; the engine runs one of {sorted(ACTS)}")
    if abs(float(eps) - 1e-5) > 1e-12:
        raise ValueError(f"{fields[2]}{where}: {eps!r}; the engine's LayerNorms are tested at 1e-5")


def _h16(t, dev):
    return t.to(H16).contiguous().to(dev)


class _Tower:
    """The blocks' weights of one tower in f16 on the device, its width and head count (None: width // 64).  Refuses before anything is moved."""

    def __init__(self, sd, prefix, dev, heads, act):
        self.width = sd[prefix + "0.ln_1.weight"].numel()
        self.heads = self.width // HEAD_DIM if heads is None else int(heads)
        _check_tower(self.width, self.heads, act, where=f" of {prefix}")
        self.layers = [{k: _h16(sd[f"{prefix}{i}.{k}"], dev) for k in _BLOCK_KEYS} for i in range(_layers(sd, prefix))]


class _Blocks:
    """The launches both engines are made of, on `dev`: GEMM, LayerNorm at `eps`, attention, and the block sequence of a _Tower with `act`."""

    def __init__(self, dev, act, eps):
        self.dev, self.L, self.act, self.eps = torch.device(dev), lib(), act, float(eps)

    def _gemm(self, x, w, bias, resid, M, act=0):
        N, K = w.shape
        y = torch.empty(M, N, dtype=H16, device=self.dev)
        self.L.tcl_gemm_f16(x, w, bias if bias is not None else 0, resid if resid is not None else 0, y, M, N, K, K, K, N, N, act, stream())
        return y

    def _ln(self, x, wb, M, C):
        y = torch.empty(M, C, dtype=H16, device=self.dev)
        self.L.tcl_layernorm_f16(x, wb[0], wb[1], y, M, C, self.eps, stream())
        return y

    def attention(self, qkv, B, T, heads, causal):
        """qkv [B*T, 3*heads*d] f16 -> [B*T, heads*d] f16 (tcl_clip_attention_f16)."""
        W = qkv.shape[1] // 3
        d = W // heads
        out = torch.empty(B * T, W, dtype=H16, device=self.dev)
        self.L.tcl_clip_attention_f16(qkv, out, B, T, heads, d, 1.0 / math.sqrt(d), int(causal), stream())
        return out

    def _blocks(self, x, tower, B, T, causal):
        M, W = B * T, tower.width
        for p in tower.layers:
            qkv = self._gemm(self._ln(x, (p["ln_1.weight"], p["ln_1.bias"]), M, W), p["attn.in_proj_weight"], p["attn.in_proj_bias"], None, M)
            x = self._gemm(self.attention(qkv, B, T, tower.heads, causal), p["attn.out_proj.weight"], p["attn.out_proj.bias"], x, M)
            u = self._gemm(self._ln(x, (p["ln_2.weight"], p["ln_2.bias"]), M, W), p["mlp.c_fc.weight"], p["mlp.c_fc.bias"], None, M, ACTS[self.act])
            if self.act == "quick_gelu":
                self.L.tcl_clip_quick_gelu_f16(u, u, u.numel(), stream())
            x = self._gemm(u, p["mlp.c_proj.weight"], p["mlp.c_proj.bias"], x, M)
        return x


class _TextTower(_Blocks):
    """A CLIP text tower on the device, from a state dict in f32 with OpenAI's names: the token table, the positional rows, the causal blocks
    (`tower`) and ln_final.  What is read off the blocks' output -- one row or all -- is its user's business."""

    def __init__(self, sd, dev, heads, act, eps):
        self.tower = _Tower(sd, "transformer.resblocks.", dev, heads, act)
        super().__init__(dev, act, eps)
        self.table, self.tpos = _h16(sd["token_embedding.weight"], self.dev), _h16(sd["positional_embedding"], self.dev)
        self.vocab, self.width = self.table.shape
        self.context = self.tpos.shape[0]
        self.ln_final = (_h16(sd["ln_final.weight"], self.dev), _h16(sd["ln_final.bias"], self.dev))
        if self.width % 64:
            raise ValueError(f"text width {self.width} must be a multiple of 64 (tcl_gemm_f16's K)")

    def blocks(self, ids):
        """ids int [B, T], 1 <= T <= context, inside the vocabulary (ValueError otherwise) -> (the rows after the last block [B*T, width] f16, B, T):
        token + positional embedding, then the causal blocks."""
        if ids.dim() != 2 or not 1 <= ids.shape[1] <= self.context:
            raise ValueError(f"token ids must be [B, T] with 1 <= T <= {self.context}, got {tuple(ids.shape)}")
        if int(ids.min()) < 0 or int(ids.max()) >= self.vocab:
            raise ValueError(f"token ids outside the vocabulary [0, {self.vocab})")
        B, T = ids.shape
        i32 = ids.to(self.dev).to(torch.int32).contiguous()
        x = torch.empty(B * T, self.width, dtype=H16, device=self.dev)
        self.L.tcl_clip_embed_f16(0, 0, i32, self.table, self.tpos, 0, 0, x, B, T, self.width, self.vocab, self.eps, stream())
        return self._blocks(x, self.tower, B, T, True), B, T


def nhwc_u8(frames):
    """Frames (numpy or tensor, any device) as a tensor, checked to be uint8 [N,H,W,3]."""
    t = frames if isinstance(frames, torch.Tensor) else torch.as_tensor(np.asarray(frames))
    if t.dim() != 4 or t.shape[-1] != 3 or t.dtype != torch.uint8:
        raise ValueError(f"frames must be uint8 [N,H,W,3], got {t.dtype} {tuple(t.shape)}")
    return t


class _ImageTower(_Blocks):
    """The image side both engines derive from: the visual `_Tower`, the patch embedding, class / positional rows, ln_pre / ln_post and the projection,
    with `preprocess`, `encode_patches` and `encode_image`.  `sd`: f32 tensors under OpenAI's `visual.*` names."""

    def __init__(self, sd, device, vision_heads, act, crop):
        if crop not in CROPS:
            raise ValueError(f"crop must be one of {sorted(CROPS)}, got {crop!r}")
        self.visual = _Tower(sd, "visual.transformer.resblocks.", device, vision_heads, act)
        super().__init__(device, act, 1e-5)
        self.crop, d = crop, self.dev
        w = sd["visual.conv1.weight"]
        self.vwidth, self.patch = w.shape[0], w.shape[-1]
        self.kpatch = 3 * self.patch * self.patch
        self.ldp = (self.kpatch + 63) // 64 * 64                                                    # patch-row stride: tcl_gemm_f16 needs K % 64 == 0
        conv1 = torch.zeros(self.vwidth, self.ldp, dtype=H16)                                       # columns kpatch .. ldp-1 zero, as the patch rows'
        conv1[:, :self.kpatch] = w.reshape(self.vwidth, -1).to(H16)                                 # [width, 3 * P * P]: (channel, row, column)
        self.conv1 = conv1.to(d)
        self.grid = int(round(math.sqrt(sd["visual.positional_embedding"].shape[0] - 1)))
        self.side = self.grid * self.patch
        self.cls, self.vpos = _h16(sd["visual.class_embedding"], d), _h16(sd["visual.positional_embedding"], d)
        self.ln_pre = (_h16(sd["visual.ln_pre.weight"], d), _h16(sd["visual.ln_pre.bias"], d))
        self.ln_post = (_h16(sd["visual.ln_post.weight"], d), _h16(sd["visual.ln_post.bias"], d))
        self.vproj = _h16(sd["visual.proj"].t(), d)                                                 # [embed, width]
        self.embed_dim = self.vproj.shape[0]
        if self.vwidth % 64:
            raise ValueError(f"vision width {self.vwidth} must be a multiple of 64 (tcl_gemm_f16's K)")

    # ---- the image encoder
    def preprocess(self, frames_u8, want_crop=False):
        """frames uint8 [N,H,W,3] (device) -> (patch rows [N*grid^2, ldp] f16 with ldp = 3*P*P rounded up to a multiple of 64 and the columns past
        3*P*P zero, the uint8 crop [N,side,side,3] or None)."""
        N, H, W = frames_u8.shape[:3]
        patches = torch.empty(N * self.grid * self.grid, self.ldp, dtype=H16, device=self.dev)
        crop = torch.empty(N, self.side, self.side, 3, dtype=torch.uint8, device=self.dev) if want_crop else None
        if self.crop == "round" and self.ldp == self.kpatch:
            self.L.tcl_clip_preprocess_u8(frames_u8, crop if want_crop else 0, patches, N, H, W, self.side, self.patch, stream())
        else:
            self.L.tcl_clip_preprocess_ld_u8(frames_u8, crop if want_crop else 0, patches, N, H, W, self.side, self.patch, self.ldp, CROPS[self.crop],
                                             stream())
        return patches, crop

    @torch.no_grad()
    def encode_patches(self, patches, B):
        """VisionTransformer.forward from the patch rows on: [B*grid^2, ldp] f16 -> features [B, embed_dim] f32."""
        T, W = self.grid * self.grid + 1, self.vwidth
        emb = self._gemm(patches, self.conv1, None, None, B * (T - 1))
        x = torch.empty(B * T, W, dtype=H16, device=self.dev)
        self.L.tcl_clip_embed_f16(emb, self.cls, 0, 0, self.vpos, self.ln_pre[0], self.ln_pre[1], x, B, T, W, 0, self.eps, stream())
        x = self._blocks(x, self.visual, B, T, False)
        c = self._ln(x.view(B, T, W)[:, 0].contiguous(), self.ln_post, B, W)
        return self._gemm(c, self.vproj, None, None, B).float()

    @torch.no_grad()
    def encode_image(self, frames_u8, batch=64):
        """CLIP.encode_image(preprocess(frame)) for uint8 frames [N,H,W,3] (numpy or tensor, any device) -> [N, embed_dim] f32 on the device."""
        t = nhwc_u8(frames_u8)
        out = []
        for s in range(0, t.shape[0], max(1, batch)):
            f = t[s:s + batch].to(self.dev).contiguous()
            patches, _ = self.preprocess(f)
            out.append(self.encode_patches(patches, f.shape[0]))
        return torch.cat(out)


class CLIPEngine(_ImageTower):
    """clip/model.py's CLIP (VisionTransformer image tower) in inference on the device.  The keyword arguments are what the tensors of a
    transformers.CLIPModel checkpoint do not say (its config.json does): the head counts (None: width // 64, OpenAI's rule), the MLP's activation
    ("quick_gelu", or "gelu" = erf, in c_fc's GEMM epilogue) and the centre-crop rule of the preprocessing ("round": clip's _transform, "floor":
    transformers' image processor).  The defaults are OpenAI's CLIP."""

    def __init__(self, state_dict, device, vision_heads=None, text_heads=None, act="quick_gelu", crop="round"):
        if crop not in CROPS:
            raise ValueError(f"crop must be one of {sorted(CROPS)}, got {crop!r}")
        missing =[k for k in ("visual.conv1.weight", "visual.proj", "token_embedding.weight", "text_projection", "ln_final.weight") if k not in state_dict]
        if missing:
            raise KeyError(f"CLIP state dict lacks {missing} (OpenAI key names; a transformers checkpoint goes through from_hf_state)")
        sd = {k: v.float() for k, v in state_dict.items() if torch.is_tensor(v)}
        super().__init__(sd, device, vision_heads, act, crop)
        d = self.dev
        self.ttower = _TextTower(sd, d, text_heads, act, self.eps)
        self.text, self.twidth, self.context = self.ttower.tower, self.ttower.width, self.ttower.context
        self.tproj = _h16(sd["text_projection"].t(), d)
        self.logit_scale = float(sd["logit_scale"]) if "logit_scale" in sd else None               # the log, as stored (CLIP.logit_scale)

    @torch.no_grad()
    def encode_text(self, ids):
        """CLIP.encode_text: ids int [B, T], 1 <= T <= context (clip.tokenize's padded layout, or tokenize_truncated's unpadded row, which uses the
        first T positional rows) -> [B, embed_dim] f32 on the device: the row of the end-of-text token, the largest id of its row."""
        ids = torch.as_tensor(ids)
        x, B, T = self.ttower.blocks(ids)
        W = self.twidth
        eot = ids.to(self.dev).argmax(-1)
        c = self._ln(x.view(B, T, W)[torch.arange(B, device=self.dev), eot].contiguous(), self.ttower.ln_final, B, W)
        return self._gemm(c, self.tproj, None, None, B).float()


VISUAL_KEYS = ("visual.conv1.weight", "visual.proj", "visual.class_embedding", "visual.positional_embedding")


def visual_state(sd):
    """The `visual.*` entries of a state dict in OpenAI's names: what CLIPVisionEngine reads of a whole CLIP (a PickScore snapshot)."""
    return {k: v for k, v in sd.items() if k.startswith("visual.")}


def from_hf_vision_state(sd):
    """`transformers.CLIPVisionModelWithProjection` names (vision_model.*, visual_projection.weight: the image_encoder of IP-Adapter) -> the
    `visual.*` part of OpenAI's names; from_hf_state's image half."""
    missing = [hf for oa, hf in _HF_TOP if oa.startswith("visual.") and hf not in sd] + [k for k in ("visual_projection.weight",) if k not in sd]
    if missing:
        raise KeyError(f"image encoder state dict lacks {missing[:3]} (transformers.CLIPVisionModelWithProjection's key names)")
    out = {oa: sd[hf] for oa, hf in _HF_TOP if oa.startswith("visual.")}
    out["visual.proj"] = sd["visual_projection.weight"].t().contiguous()
    oa, hf = _HF_TOWERS[0]
    _tower_from_hf(out, sd.__getitem__, _layers(sd, hf), oa, hf)
    return out


class CLIPVisionEngine(_ImageTower):
    """The image tower of CLIPEngine alone (`transformers.CLIPVisionModelWithProjection`: `encode_image` returns its projected, un-normalised
    image_embeds): what IP-Adapter conditions on.  The state dict holds the `visual.*` keys in OpenAI's names; a text tower is neither needed nor read."""

    def __init__(self, state_dict, device, vision_heads=None, act="quick_gelu", crop="round"):
        missing = [k for k in VISUAL_KEYS if k not in state_dict]
        if missing:
            raise KeyError(f"CLIP image tower state dict lacks {missing} (OpenAI key names; a transformers checkpoint goes through from_hf_vision_state)")
        super().__init__({k: v.float() for k, v in visual_state(state_dict).items() if torch.is_tensor(v)}, device, vision_heads, act, crop)


def vision_options(config=None, vision_width=None, patch=None):
    """CLIPVisionEngine's keyword arguments for the CLIP ViT-H/14 image tower: from the dictionary of a config.json -- a CLIPVisionConfig (the fields at
    the top level) or a CLIPConfig (under vision_config: a PickScore snapshot) -- else PICKSCORE_V1's.  The rules, and what is refused, are
    pick_options' for the vision tower."""
    A, D = PICKSCORE_V1, _HF_DEFAULTS
    vc = to_hf_config(A)["vision_config"] if config is None else (config.get("vision_config") or config)
    heads, act = vc.get("num_attention_heads", D["num_attention_heads"][0]), vc.get("hidden_act", D["hidden_act"])
    _check_tower(vision_width or A["vision_width"], heads, act, vc.get("layer_norm_eps", D["layer_norm_eps"]), (64, 80), _HF_FIELDS, " (vision)")
    psz = vc.get("patch_size", D["patch_size"])
    if patch is not None and int(psz) != int(patch):
        raise ValueError(f"patch_size {psz!r} of the config, but the checkpoint's patch embedding is {patch} x {patch}")
    return dict(vision_heads=int(heads), act=act, crop="floor")


def vision_engine(state, device, config=None):
    """The CLIPVisionEngine of IP-Adapter-SD1.5's image encoder (CLIP ViT-H/14) from a state dict in OpenAI's names (model_utils.load_image_encoder_state:
    a vision snapshot's, or the visual.* part of a PickScore one) and the snapshot's config.json dictionary: the tower pick_engine builds, alone."""
    if "visual.conv1.weight" not in state:
        raise KeyError("image encoder state dict lacks visual.conv1.weight (OpenAI key names; see from_hf_vision_state)")
    w = state["visual.conv1.weight"]
    return CLIPVisionEngine(state, device, **vision_options(config, w.shape[0], w.shape[-1]))


class CLIPTextEngine(_TextTower):
    """A CLIP text tower alone, read at every position: `transformers.CLIPTextModel(...).last_hidden_state`, what SD-1.5 conditions its UNet on
    (SD15_TEXT: the text tower of CLIP ViT-L/14).  The state dict holds token_embedding.weight, positional_embedding, transformer.resblocks.* and
    ln_final.* in OpenAI's names (a transformers checkpoint goes through from_hf_text_state); a text_projection or an image tower is not needed and
    not read.  heads None: width // 64; act: "quick_gelu" or "gelu"; eps: the LayerNorms'."""

    def __init__(self, state_dict, device, heads=None, act="quick_gelu", eps=1e-5):
        missing = [k for k in ("token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias") if k not in state_dict]
        if missing:
            raise KeyError(f"CLIP text state dict lacks {missing} (OpenAI key names; a transformers checkpoint goes through from_hf_text_state)")
        super().__init__({k: v.float() for k, v in state_dict.items() if torch.is_tensor(v)}, device, heads, act, eps)

    @torch.no_grad()
    def hidden_states(self, ids):
        """ids int [B, T], 1 <= T <= context -> [B, T, width] f16 on the device: token + positional embedding, the causal blocks, ln_final on every
        row; no projection and no pooling.  Row t depends on ids[:, :t + 1] only."""
        x, B, T = self.blocks(torch.as_tensor(ids))
        return self._ln(x, self.ln_final, B * T, self.width).view(B, T, self.width)


def scores(feats, text=None):
    """feats [N,D] f32 (device), text [D] f32 or None -> (clip-frame, clip-text or None) as Python floats (tcl_clip_scores: f64, fixed order)."""
    f = feats.float().contiguous()
    N, D = f.shape
    L = lib()
    t = text.float().contiguous().view(-1) if text is not None else None
    if t is not None and t.numel() != D:
        raise ValueError(f"text feature must have {D} elements, got {t.numel()}")
    out = torch.empty(2, dtype=torch.float64, device=f.device)
    ws = torch.empty(L.tcl_clip_scores_workspace_bytes(N), dtype=torch.uint8, device=f.device)
    L.tcl_clip_scores(f, t if t is not None else 0, N, D, out, ws, stream())
    o = out.cpu().tolist()
    return o[0], (o[1] if t is not None else None)


def pick_scores(feats, text, logit_scale):
    """pick_score_func (eval_utils.py:163-176): feats [N,D] f32 (device), text [D] f32, logit_scale (the log) -> (the mean score as a Python float,
    the per-image scores exp(logit_scale) cos(text, feat_i) as a float64 numpy array).  tcl_pick_scores: f64, fixed order."""
    f = feats.float().contiguous()
    N, D = f.shape
    t = text.float().contiguous().view(-1)
    if t.numel() != D:
        raise ValueError(f"text feature must have {D} elements, got {t.numel()}")
    out = torch.empty(N + 1, dtype=torch.float64, device=f.device)
    lib().tcl_pick_scores(f, t.to(f.device), N, D, float(logit_scale), out, stream())
    o = out.cpu().numpy()
    return float(o[0]), o[1:]


_HF_DEFAULTS = dict(num_attention_heads=(12, 8), hidden_act="quick_gelu", layer_norm_eps=1e-5, patch_size=32)     # transformers' CLIP*Config


def pick_options(config=None, vision_width=None, text_width=None, patch=None):
    """CLIPEngine's keyword arguments for the PickScore model: from `config`, the dictionary of a transformers config.json (vision_config /
    text_config: num_attention_heads, hidden_act, layer_norm_eps, patch_size; a field that is absent has transformers' default), else PICKSCORE_V1.
    ValueError, naming the field, for what the kernels do not cover: an activation other than quick_gelu / gelu, a head_dim outside {64, 80}, a
    LayerNorm eps other than 1e-5, and a patch_size that is not the checkpoint's.  Host-side: no device is touched."""
    A, D = PICKSCORE_V1, _HF_DEFAULTS
    vw, tw = vision_width or A["vision_width"], text_width or A["transformer_width"]
    config = to_hf_config(A) if config is None else config
    vc, tc = config.get("vision_config") or {}, config.get("text_config") or {}
    heads = (vc.get("num_attention_heads", D["num_attention_heads"][0]), tc.get("num_attention_heads", D["num_attention_heads"][1]))
    acts = (vc.get("hidden_act", D["hidden_act"]), tc.get("hidden_act", D["hidden_act"]))
    eps = (vc.get("layer_norm_eps", D["layer_norm_eps"]), tc.get("layer_norm_eps", D["layer_norm_eps"]))
    psz = vc.get("patch_size", D["patch_size"])
    if acts[0] != acts[1]:
        raise ValueError(f"hidden_act {acts[0]!r} (vision) / {acts[1]!r} (text): the engine runs one activation in both towers")
    for tower, w, h, a, e in zip(("vision", "text"), (vw, tw), heads, acts, eps):                 # head_dim 64 / 80: what the engine is tested at
        _check_tower(w, h, a, e, (64, 80), _HF_FIELDS, f" ({tower})")
    if patch is not None and int(psz) != int(patch):
        raise ValueError(f"patch_size {psz!r} of the config, but the checkpoint's patch embedding is {patch} x {patch}")
    return dict(vision_heads=int(heads[0]), text_heads=int(heads[1]), act=acts[0], crop="floor")


def to_hf_config(arch, vision_layers=None, text_layers=None):
    """An architecture dictionary (PICKSCORE_V1) as the dictionary of a transformers config.json (`CLIPConfig(**to_hf_config(arch))`): the inverse of
    pick_options' reading, used by the goldens and the tests.  The layer counts can be overridden for small models of the same widths."""
    act, eps = arch.get("act", "quick_gelu"), arch.get("eps", 1e-5)
    vision = dict(hidden_size=arch["vision_width"], intermediate_size=4 * arch["vision_width"], image_size=arch["image_resolution"],
                  num_hidden_layers=vision_layers or arch["vision_layers"], patch_size=arch["vision_patch_size"], projection_dim=arch["embed_dim"],
                  num_attention_heads=arch.get("vision_heads", arch["vision_width"] // HEAD_DIM), hidden_act=act, layer_norm_eps=eps)
    text = dict(hidden_size=arch["transformer_width"], intermediate_size=4 * arch["transformer_width"], vocab_size=arch["vocab_size"],
                num_hidden_layers=text_layers or arch["transformer_layers"], max_position_embeddings=arch["context_length"],
                projection_dim=arch["embed_dim"], num_attention_heads=arch.get("text_heads", arch["transformer_width"] // HEAD_DIM), hidden_act=act,
                layer_norm_eps=eps, bos_token_id=SOT, eos_token_id=EOT)
    return dict(vision_config=vision, text_config=text, projection_dim=arch["embed_dim"], logit_scale_init_value=math.log(1 / 0.07))


_HF_TEXT_DEFAULTS = dict(hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8, max_position_embeddings=77,
                         hidden_act="quick_gelu", layer_norm_eps=1e-5)                                    # transformers' CLIPTextConfig


def text_options(config=None):
    """CLIPTextEngine's keyword arguments from the dictionary of a text_encoder's config.json (num_attention_heads, hidden_act, layer_norm_eps,
    hidden_size, intermediate_size; a field that is absent has transformers' default) -> (dict(heads, act, eps), the shape the config promises:
    dict(width, layers, context_length)).  ValueError, naming the field, for what the kernels do not cover: a head_dim that is not a multiple of 16
    or is above 128, an activation other than quick_gelu / gelu, a LayerNorm eps other than 1e-5, an intermediate_size other than 4 x hidden_size.
    Host-side: no device is touched."""
    c = dict(_HF_TEXT_DEFAULTS, **{k: v for k, v in (config or {}).items() if k in _HF_TEXT_DEFAULTS})
    w, h = c["hidden_size"], c["num_attention_heads"]
    if not isinstance(w, int) or w <= 0 or w % 64:
        raise ValueError(f"hidden_size {w!r}: the width must be a positive multiple of 64 (tcl_gemm_f16's K)")
    _check_tower(w, h, c["hidden_act"], c["layer_norm_eps"], fields=_HF_FIELDS)
    if c["intermediate_size"] != 4 * w:
        raise ValueError(f"intermediate_size {c['intermediate_size']!r}: the MLP must be 4 x hidden_size = {4 * w} wide")
    return (dict(heads=h, act=c["hidden_act"], eps=1e-5),
            dict(width=w, layers=c["num_hidden_layers"], context_length=c["max_position_embeddings"]))


def to_hf_text_config(arch):
    """A text architecture dictionary (SD15_TEXT) as the dictionary of a transformers config.json (`CLIPTextConfig(**to_hf_text_config(arch))`): the
    inverse of text_options' reading, used by the golden and the tests."""
    w = arch["width"]
    return dict(hidden_size=w, intermediate_size=4 * w, num_hidden_layers=arch["layers"], num_attention_heads=arch.get("heads") or w // HEAD_DIM,
                max_position_embeddings=arch["context_length"], vocab_size=arch["vocab_size"], hidden_act=arch.get("act", "quick_gelu"),
                layer_norm_eps=arch.get("eps", 1e-5), projection_dim=w, bos_token_id=arch["vocab_size"] - 2, eos_token_id=arch["vocab_size"] - 1)


def pick_engine(state, device, config=None):
    """The CLIPEngine of PickScore_v1 from a state dict in OpenAI's key names (model_utils.load_pick_state) and, when there is one, the checkpoint's
    config.json dictionary: GELU, 16 heads per tower, the transformers processor's crop.  See pick_options for what is refused."""
    if "visual.conv1.weight" not in state or "positional_embedding" not in state:
        raise KeyError("PickScore state dict lacks visual.conv1.weight / positional_embedding (OpenAI key names; see from_hf_state)")
    w = state["visual.conv1.weight"]
    return CLIPEngine(state, device, **pick_options(config, w.shape[0], state["positional_embedding"].shape[1], w.shape[-1]))


def useful_flops(engine, n_images=1):
    """Multiply-adds x 2 of encode_image for n images: the patch GEMM (its 3 P^2 real columns, not the zero padding), the blocks (in_proj, QK^T and
    PV -- 4 T^2 W whatever the head count --, out_proj, the MLP) with T = grid^2 + 1, and the projection."""
    W, T, Lr = engine.vwidth, engine.grid ** 2 + 1, len(engine.visual.layers)
    per = 2 * (T - 1) * W * 3 * engine.patch ** 2 + Lr * (2 * T * W * 3 * W + 4 * T * T * W + 2 * T * W * W + 16 * T * W * W) + 2 * W * engine.embed_dim
    return per * n_images
