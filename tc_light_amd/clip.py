"""OpenAI CLIP on the device: the model behind the clip-frame and clip-text figures of the reference's evaluate.py (evaluate.py:119
`clip.load("ViT-B/32")`; utils/evaluation/eval_utils.py:129-161).

`CLIPEngine` = clip/model.py's CLIP in inference: `encode_image` is `preprocess` (Resize(BICUBIC) -> CenterCrop -> ToTensor -> Normalize, one kernel on
the uint8 frames) -> conv1 as a GEMM over patch rows -> [class | patches] + positional embedding -> ln_pre -> the pre-LN residual blocks -> ln_post on
the class token -> proj; `encode_text` is token + positional embedding -> the same blocks with the causal mask -> ln_final on the row of the
end-of-text token (`ids.argmax(-1)`) -> text_projection.  A block is LayerNorm, the fused in_proj GEMM, tcl_clip_attention_f16 (which reads the GEMM's
[q | k | v] rows in place), out_proj with the residual in its epilogue, LayerNorm, c_fc, QuickGELU, c_proj with the residual.  Widths, depth, patch
size and context length come from the tensor shapes and the head count is width // 64 (clip/model.py build_model), so another CLIP of this family
loads unchanged.  Activations are f16 with f32 accumulation; the features are returned as f32.

State dicts use OpenAI's key names.  `from_hf_state` / `to_hf_state` map to and from `transformers.CLIPModel`'s names (q / k / v concatenated into
in_proj, the projections transposed).  Pinned against `transformers.CLIPModel` in f32 by tests/golden/clip.npz (tests/test_gpu_clip.py).
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


# ---- state dicts
def _block_shapes(sh, prefix, width):
    sh[prefix + "attn.in_proj_weight"] = (3 * width, width); sh[prefix + "attn.in_proj_bias"] = (3 * width,)
    sh[prefix + "attn.out_proj.weight"] = (width, width); sh[prefix + "attn.out_proj.bias"] = (width,)
    sh[prefix + "ln_1.weight"] = (width,); sh[prefix + "ln_1.bias"] = (width,)
    sh[prefix + "mlp.c_fc.weight"] = (4 * width, width); sh[prefix + "mlp.c_fc.bias"] = (4 * width,)
    sh[prefix + "mlp.c_proj.weight"] = (width, 4 * width); sh[prefix + "mlp.c_proj.bias"] = (width,)
    sh[prefix + "ln_2.weight"] = (width,); sh[prefix + "ln_2.bias"] = (width,)


def clip_param_shapes(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32, context_length=77,
                      vocab_size=49408, transformer_width=512, transformer_layers=12):
    """State-dict keys and shapes of clip/model.py's CLIP with a VisionTransformer tower (the defaults are ViT-B/32)."""
    sh = {}
    vw, tw = vision_width, transformer_width
    grid = image_resolution // vision_patch_size
    sh["visual.class_embedding"] = (vw,)
    sh["visual.positional_embedding"] = (grid * grid + 1, vw)
    sh["visual.conv1.weight"] = (vw, 3, vision_patch_size, vision_patch_size)
    sh["visual.ln_pre.weight"] = (vw,); sh["visual.ln_pre.bias"] = (vw,)
    for i in range(vision_layers):
        _block_shapes(sh, f"visual.transformer.resblocks.{i}.", vw)
    sh["visual.ln_post.weight"] = (vw,); sh["visual.ln_post.bias"] = (vw,)
    sh["visual.proj"] = (vw, embed_dim)
    sh["token_embedding.weight"] = (vocab_size, tw)
    sh["positional_embedding"] = (context_length, tw)
    for i in range(transformer_layers):
        _block_shapes(sh, f"transformer.resblocks.{i}.", tw)
    sh["ln_final.weight"] = (tw,); sh["ln_final.bias"] = (tw,)
    sh["text_projection"] = (tw, embed_dim)
    sh["logit_scale"] = ()
    return sh


def seeded_state_dict(seed=6, **arch):
    """Seeded stand-in weights of the architecture (default ViT-B/32), scaled so that the features depend on the input -- with the usual small
    initialisation the class token barely hears the patches and every image gets almost the same feature.  Linears are N(0, g^2 / fan_in) with
    g = 1 for in_proj (attention logits of about one unit: the softmax selects) and the MLP's c_fc, and 0.7 for the two output projections of a
    block; LayerNorm weights 1 +- 0.1, biases +- 0.1; embeddings N(0, 1) (class / positional at 0.3); the columns of the two final projections
    decay as 0.75^j, so a feature lives mostly in a few directions and cosines between features of unrelated inputs spread over [-1, 1]."""
    shapes = clip_param_shapes(**arch)
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


def to_hf_state(sd):
    """OpenAI names -> `transformers.CLIPModel` names: in_proj split into q / k / v, `visual.proj` / `text_projection` transposed into Linear weights."""
    out = {hf: sd[oa] for oa, hf in _HF_TOP}
    out["visual_projection.weight"] = sd["visual.proj"].t().contiguous()
    out["text_projection.weight"] = sd["text_projection"].t().contiguous()
    for oa, hf in _HF_TOWERS:
        for i in range(_layers(sd, oa)):
            a, h = f"{oa}{i}.", f"{hf}{i}."
            for kind in ("weight", "bias"):
                q, k, v = sd[a + "attn.in_proj_" + kind].chunk(3, 0)
                out[h + "self_attn.q_proj." + kind], out[h + "self_attn.k_proj." + kind], out[h + "self_attn.v_proj." + kind] = \
                    q.contiguous(), k.contiguous(), v.contiguous()
                for x, y in _HF_BLOCK:
                    out[h + y + kind] = sd[a + x + kind]
    return out


def from_hf_state(sd):
    """`transformers.CLIPModel` names -> OpenAI names (the inverse of to_hf_state; `position_ids` buffers of older checkpoints are dropped)."""
    out = {oa: sd[hf] for oa, hf in _HF_TOP}
    out["visual.proj"] = sd["visual_projection.weight"].t().contiguous()
    out["text_projection"] = sd["text_projection.weight"].t().contiguous()
    for oa, hf in _HF_TOWERS:
        for i in range(_layers(sd, hf)):
            a, h = f"{oa}{i}.", f"{hf}{i}."
            for kind in ("weight", "bias"):
                out[a + "attn.in_proj_" + kind] = torch.cat([sd[h + f"self_attn.{n}_proj." + kind] for n in "qkv"]).contiguous()
                for x, y in _HF_BLOCK:
                    out[a + x + kind] = sd[h + y + kind]
    return out


# ---- geometry and tokens
def resize_geometry(H, W, side=224):
    """The sizes of clip's `_transform(side)` for an H x W frame -> (resized height, resized width, crop top, crop left): Resize puts the short side at
    `side` and the long one at int(side * long / short); CenterCrop starts at int(round((size - side) / 2.0)).  (tcl_clip_resize_geometry is the
    same rule on the C side.)"""
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(side * long_ / short)
    oh, ow = (new_long, side) if W <= H else (side, new_long)
    return oh, ow, int(round((oh - side) / 2.0)), int(round((ow - side) / 2.0))


def _stand_in_ids(text, room):
    seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:4], "little")
    n = min(room, max(1, len(text.replace(",", " , ").replace(".", " . ").split())))
    return np.random.default_rng(seed).integers(1000, 40000, n).tolist()


def tokenize(prompt, tokenizer, context=77, allow_random=False):
    """clip.tokenize([prompt]) from any tokenizer with the HF CLIP interface (`tokenizer(txt, truncation=False, add_special_tokens=False)["input_ids"]`,
    `.bos_token_id`, `.eos_token_id`): int64 [1, context] = [SOT] + ids + [EOT], zero-padded.  RuntimeError when the prompt does not fit, as
    clip.tokenize raises (the caller then splits on '.', evaluate.py:43-49).  tokenizer None: an error unless `allow_random`, which gives a
    deterministic text-seeded id sequence (one id per word) with a warning."""
    if tokenizer is None:
        if not allow_random:
            raise FileNotFoundError("no CLIP tokenizer (models.clip_tokenizer / --clip_tokenizer); set models.allow_random / "
                                    "TCL_ALLOW_RANDOM_WEIGHTS=1 for deterministic stand-in token ids")
        warnings.warn("CLIP tokenizer not found -> deterministic text-seeded stand-in token ids (allow_random)")
        ids, sot, eot = _stand_in_ids(prompt, 10 ** 9), SOT, EOT
    else:
        ids = list(tokenizer(prompt, truncation=False, add_special_tokens=False)["input_ids"])
        sot, eot = int(tokenizer.bos_token_id), int(tokenizer.eos_token_id)
    if len(ids) + 2 > context:
        raise RuntimeError(f"Input {prompt!r} is too long for context length {context}")
    out = torch.zeros(1, context, dtype=torch.int64)
    out[0, :len(ids) + 2] = torch.tensor([sot] + ids + [eot], dtype=torch.int64)
    return out


def load_tokenizer(tok_dir):
    """A CLIPTokenizer from a local directory (the directory itself or its `tokenizer` sub-directory), or None when there is none."""
    import os
    for d in (tok_dir, os.path.join(tok_dir, "tokenizer") if tok_dir else None):
        if d and os.path.isfile(os.path.join(d, "vocab.json")):
            from transformers import CLIPTokenizer
            return CLIPTokenizer.from_pretrained(d)
    return None


# ---- the engine
class _Tower:
    def __init__(self, sd, prefix, dev):
        self.layers = []
        for i in range(_layers(sd, prefix)):
            p = f"{prefix}{i}."
            self.layers.append({k: sd[p + k].to(H16).contiguous().to(dev) for k in (
                "ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")})
        self.width = self.layers[0]["ln_1.weight"].numel()
        self.heads = self.width // HEAD_DIM


class CLIPEngine:
    """clip/model.py's CLIP (VisionTransformer image tower) in inference on the device."""

    def __init__(self, state_dict, device):
        missing = [k for k in ("visual.conv1.weight", "visual.proj", "token_embedding.weight", "text_projection", "ln_final.weight") if k not in state_dict]
        if missing:
            raise KeyError(f"CLIP state dict lacks {missing} (OpenAI key names; a transformers checkpoint goes through from_hf_state)")
        self.dev, self.L = torch.device(device), lib()
        sd = {k: v.float() for k, v in state_dict.items() if torch.is_tensor(v)}
        d = self.dev

        def h(k):
            return sd[k].to(H16).contiguous().to(d)

        w = sd["visual.conv1.weight"]
        self.vwidth, self.patch = w.shape[0], w.shape[-1]
        self.conv1 = w.reshape(self.vwidth, -1).to(H16).contiguous().to(d)                          # [width, 3 * P * P]: (channel, row, column)
        self.grid = int(round(math.sqrt(sd["visual.positional_embedding"].shape[0] - 1)))
        self.side = self.grid * self.patch
        self.cls, self.vpos = h("visual.class_embedding"), h("visual.positional_embedding")
        self.ln_pre = (h("visual.ln_pre.weight"), h("visual.ln_pre.bias"))
        self.ln_post = (h("visual.ln_post.weight"), h("visual.ln_post.bias"))
        self.vproj = sd["visual.proj"].t().to(H16).contiguous().to(d)                               # [embed, width]
        self.visual = _Tower(sd, "visual.transformer.resblocks.", d)
        self.table, self.tpos = h("token_embedding.weight"), h("positional_embedding")
        self.vocab, self.twidth = self.table.shape
        self.context = self.tpos.shape[0]
        self.ln_final = (h("ln_final.weight"), h("ln_final.bias"))
        self.tproj = sd["text_projection"].t().to(H16).contiguous().to(d)
        self.text = _Tower(sd, "transformer.resblocks.", d)
        self.embed_dim = self.vproj.shape[0]
        if (3 * self.patch * self.patch) % 64 or self.vwidth % 64 or self.twidth % 64:
            raise ValueError(f"widths {self.vwidth} / {self.twidth} and 3 * patch^2 = {3 * self.patch ** 2} must be multiples of 64 (tcl_gemm_f16's K)")

    # ---- building blocks
    def _gemm(self, x, w, bias, resid, M):
        N, K = w.shape
        y = torch.empty(M, N, dtype=H16, device=self.dev)
        self.L.tcl_gemm_f16(x, w, bias if bias is not None else 0, resid if resid is not None else 0, y, M, N, K, K, K, N, N, 0, stream())
        return y

    def _ln(self, x, wb, M, C):
        y = torch.empty(M, C, dtype=H16, device=self.dev)
        self.L.tcl_layernorm_f16(x, wb[0], wb[1], y, M, C, 1e-5, stream())
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
            u = self._gemm(self._ln(x, (p["ln_2.weight"], p["ln_2.bias"]), M, W), p["mlp.c_fc.weight"], p["mlp.c_fc.bias"], None, M)
            self.L.tcl_clip_quick_gelu_f16(u, u, u.numel(), stream())
            x = self._gemm(u, p["mlp.c_proj.weight"], p["mlp.c_proj.bias"], x, M)
        return x

    # ---- the two encoders
    def preprocess(self, frames_u8, want_crop=False):
        """frames uint8 [N,H,W,3] (device) -> (patch rows [N*grid^2, 3*P*P] f16, the uint8 crop [N,side,side,3] or None)."""
        N, H, W = frames_u8.shape[:3]
        patches = torch.empty(N * self.grid * self.grid, 3 * self.patch * self.patch, dtype=H16, device=self.dev)
        crop = torch.empty(N, self.side, self.side, 3, dtype=torch.uint8, device=self.dev) if want_crop else None
        self.L.tcl_clip_preprocess_u8(frames_u8, crop if want_crop else 0, patches, N, H, W, self.side, self.patch, stream())
        return patches, crop

    @torch.no_grad()
    def encode_patches(self, patches, B):
        """VisionTransformer.forward from the patch rows on: [B*grid^2, 3*P*P] f16 -> features [B, embed_dim] f32."""
        T, W = self.grid * self.grid + 1, self.vwidth
        emb = self._gemm(patches, self.conv1, None, None, B * (T - 1))
        x = torch.empty(B * T, W, dtype=H16, device=self.dev)
        self.L.tcl_clip_embed_f16(emb, self.cls, 0, 0, self.vpos, self.ln_pre[0], self.ln_pre[1], x, B, T, W, 0, 1e-5, stream())
        x = self._blocks(x, self.visual, B, T, False)
        c = self._ln(x.view(B, T, W)[:, 0].contiguous(), self.ln_post, B, W)
        return self._gemm(c, self.vproj, None, None, B).float()

    @torch.no_grad()
    def encode_image(self, frames_u8, batch=64):
        """CLIP.encode_image(preprocess(frame)) for uint8 frames [N,H,W,3] (numpy or tensor, any device) -> [N, embed_dim] f32 on the device."""
        t = frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.as_tensor(np.asarray(frames_u8))
        if t.dim() != 4 or t.shape[-1] != 3 or t.dtype != torch.uint8:
            raise ValueError(f"frames must be uint8 [N,H,W,3], got {t.dtype} {tuple(t.shape)}")
        out = []
        for s in range(0, t.shape[0], max(1, batch)):
            f = t[s:s + batch].to(self.dev).contiguous()
            patches, _ = self.preprocess(f)
            out.append(self.encode_patches(patches, f.shape[0]))
        return torch.cat(out)

    @torch.no_grad()
    def encode_text(self, ids):
        """CLIP.encode_text: ids int [B, context] (clip.tokenize's layout) -> [B, embed_dim] f32 on the device."""
        ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.shape[1] != self.context:
            raise ValueError(f"token ids must be [B, {self.context}], got {tuple(ids.shape)}")
        if int(ids.min()) < 0 or int(ids.max()) >= self.vocab:
            raise ValueError(f"token ids outside the vocabulary [0, {self.vocab})")
        B, T, W = ids.shape[0], self.context, self.twidth
        i32 = ids.to(self.dev).to(torch.int32).contiguous()
        x = torch.empty(B * T, W, dtype=H16, device=self.dev)
        self.L.tcl_clip_embed_f16(0, 0, i32, self.table, self.tpos, 0, 0, x, B, T, W, self.vocab, 1e-5, stream())
        x = self._blocks(x, self.text, B, T, True)
        eot = ids.to(self.dev).argmax(-1)
        c = self._ln(x.view(B, T, W)[torch.arange(B, device=self.dev), eot].contiguous(), self.ln_final, B, W)
        return self._gemm(c, self.tproj, None, None, B).float()


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


def useful_flops(engine, n_images=1):
    """Multiply-adds x 2 of encode_image for n images: the patch GEMM, the blocks (in_proj, QK^T and PV, out_proj, the MLP) and the projection."""
    W, T, Lr = engine.vwidth, engine.grid ** 2 + 1, len(engine.visual.layers)
    per = 2 * (T - 1) * W * 3 * engine.patch ** 2 + Lr * (2 * T * W * 3 * W + 4 * T * T * W + 2 * T * W * W + 16 * T * W * W) + 2 * W * engine.embed_dim
    return per * n_images
