"""IP-Adapter for SD-1.5 (Ye et al. 2023, "IP-Adapter: Text Compatible Image Prompt Adapter for Text-to-Image Diffusion Models") on the IC-Light
UNet: generation.ip_adapter relights towards a reference image.

The adapter is a projection of the CLIP ViT-H/14 image embedding to 4 tokens of the text width,
    tokens = LayerNorm(proj(image_embeds).view(4, 768)),
and, beside every text cross-attention (attn2) of the UNet, one more key / value pair to_k_ip / to_v_ip reading those tokens:
    attn2(x) = Attention(q, K_text, V_text) + scale * Attention(q, K_ip, V_ip)                         (the paper's eq. 5, one q for both).
The unconditional half of classifier-free guidance gets the tokens of a ZERO image embedding.

File layout (ip-adapter_sd15.safetensors, or the .bin it was converted from: {"image_proj": {...}, "ip_adapter": {...}}):
    image_proj.proj.weight [4 * 768, 1024], image_proj.proj.bias [4 * 768], image_proj.norm.weight / .bias [768]
    ip_adapter.<i>.to_k_ip.weight / ip_adapter.<i>.to_v_ip.weight [C, 768] for the odd i = 1, 3 .. 31
The odd indices are the attn2 processors in diffusers' `unet.attn_processors` order: the down blocks (1, 3 -> 320; 5, 7 -> 640; 9, 11 -> 1280), then
the up blocks (13, 15, 17 -> 1280; 19, 21, 23 -> 640; 25, 27, 29 -> 320), then the mid block (31 -> 1280): `BLOCK_OF_INDEX`.  That order is restated
from memory of the published file and is NOT verified against one (no checkpoint was at hand); every shape is checked against the width of the
block it lands on, which catches any order that moves a tensor between widths, and the "plus" files (16 tokens, a Resampler: image_proj.latents) are
refused by name.

`load_state` reads and checks a file, `image_tokens` runs the projection on the existing kernels (tcl_gemm_f16, tcl_layernorm_f16), `image_embeds` runs
the reference image through the CLIP ViT-H/14 image tower (clip.vision_engine: the PIL-exact preprocess with the transformers processor's crop) and
frees it, `build` puts them together into the unet.ImagePrompt the Generator hands to every xy pass.
"""
import os

import numpy as np
import torch

from . import sd15

H16 = torch.float16
N_TOKENS, TOKEN_DIM, EMBED_DIM = 4, 768, 1024            # ip-adapter_sd15: 4 tokens of SD-1.5's text width from CLIP ViT-H/14's image_embeds


def _block_of_index():
    out, i = {}, 1
    order = [f"down_blocks.{b}.attentions.{j}." for b in range(3) for j in range(2)] \
        + [f"up_blocks.{b}.attentions.{j}." for b in (1, 2, 3) for j in range(3)] + ["mid_block.attentions.0."]
    for p in order:
        out[i] = p
        i += 2
    return out


BLOCK_OF_INDEX = _block_of_index()                       # odd processor index of the file -> this engine's transformer block prefix


def block_widths():
    """{transformer block prefix: C} of the SD-1.5 UNet (the shapes of attn2.to_q)."""
    sh = sd15.unet_param_shapes()
    return {p: sh[p + "transformer_blocks.0.attn2.to_q.weight"][0] for p in BLOCK_OF_INDEX.values()}


def param_shapes():
    """Keys and shapes of ip-adapter_sd15 in the flat (safetensors) spelling."""
    sh = {"image_proj.proj.weight": (N_TOKENS * TOKEN_DIM, EMBED_DIM), "image_proj.proj.bias": (N_TOKENS * TOKEN_DIM,),
          "image_proj.norm.weight": (TOKEN_DIM,), "image_proj.norm.bias": (TOKEN_DIM,)}
    widths = block_widths()
    for i, p in BLOCK_OF_INDEX.items():
        sh[f"ip_adapter.{i}.to_k_ip.weight"] = (widths[p], TOKEN_DIM)
        sh[f"ip_adapter.{i}.to_v_ip.weight"] = (widths[p], TOKEN_DIM)
    return sh


def seeded_state_dict(seed=10):
    """Seeded stand-in weights in the published layout: Linears N(0, 1 / fan_in), the LayerNorm 1 +- 0.1 / +- 0.1."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in param_shapes().items():
        r = torch.randn(*s, generator=g)
        if k == "image_proj.norm.weight":
            sd[k] = 1.0 + 0.1 * r
        elif k.endswith("bias"):
            sd[k] = 0.1 * r
        else:
            sd[k] = r / float(s[1]) ** 0.5
    return sd


def to_nested(sd):
    """The flat spelling -> the .bin's {"image_proj": {...}, "ip_adapter": {...}}."""
    out = {"image_proj": {}, "ip_adapter": {}}
    for k, v in sd.items():
        top, rest = k.split(".", 1)
        out[top][rest] = v
    return out


def read_file(path):
    """ip-adapter_sd15.safetensors (flat keys) or .bin (a pickled {"image_proj": {...}, "ip_adapter": {...}}) -> flat {name: tensor} on the CPU."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return dict(load_file(path))
    raw = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(raw, dict):
        raise ValueError(f"IP-Adapter file {path!r}: expected a dictionary of tensors, got {type(raw).__name__}")
    flat = {}
    for k, v in raw.items():
        if isinstance(v, dict):
            flat.update({f"{k}.{kk}": vv for kk, vv in v.items()})
        else:
            flat[k] = v
    return flat


def check_state(sd):
    """A flat state dict -> (proj, weights): proj = {weight [3072, 1024], bias, norm_weight, norm_bias} f32 and weights = {transformer block prefix:
    [2C, 768] f32 = to_k_ip ; to_v_ip}.  ValueError naming the key (and both shapes) for a tensor that is missing or is not the shape its target
    block takes, and for the "plus" variants, which this engine does not run."""
    plus = [k for k in sd if k.startswith("image_proj.latents") or k.startswith("image_proj.layers.") or k.startswith("image_proj.proj_in")]
    if plus:
        raise ValueError(f"IP-Adapter file holds {plus[0]}: a 'plus' variant (16 tokens from a Resampler over the penultimate hidden states) is not "
                         "supported; use ip-adapter_sd15 (4 tokens from image_embeds)")
    want = param_shapes()
    for k, s in want.items():
        if k not in sd:
            raise ValueError(f"IP-Adapter state dict lacks {k} (expected shape {tuple(s)})")
        if tuple(sd[k].shape) != tuple(s):
            where = ""
            if k.startswith("ip_adapter."):
                where = f" of block {BLOCK_OF_INDEX[int(k.split('.')[1])]}"
            raise ValueError(f"IP-Adapter {k} has shape {tuple(sd[k].shape)}, expected {tuple(s)}{where}")
    proj = dict(weight=sd["image_proj.proj.weight"].float(), bias=sd["image_proj.proj.bias"].float(),
                norm_weight=sd["image_proj.norm.weight"].float(), norm_bias=sd["image_proj.norm.bias"].float())
    weights = {p: torch.cat([sd[f"ip_adapter.{i}.to_k_ip.weight"].float(), sd[f"ip_adapter.{i}.to_v_ip.weight"].float()])
               for i, p in BLOCK_OF_INDEX.items()}
    return proj, weights


def load_state(path=None, seed=10, allow=False):
    """models.ip_adapter / generation.ip_adapter.path -> check_state's (proj, weights).  A missing file is a FileNotFoundError unless `allow`
    (models.allow_random), which stands seeded tensors in -- the rule every other model follows (model_utils._missing)."""
    from .model_utils import _missing
    if not (path and os.path.isfile(path)):
        _missing("IP-Adapter", path, allow)
        return check_state(seeded_state_dict(seed))
    return check_state(read_file(path))


def read_image_u8(path):
    """The reference image -> uint8 [1, H, W, 3] (RGB)."""
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8).copy())[None]


@torch.no_grad()
def image_tokens(embeds, proj, dev):
    """embeds [1024] (the projected, un-normalised image_embeds) -> tokens [2, 4, 768] f16 on `dev`: entry 0 from a zero embedding (IP-Adapter's
    unconditional image), entry 1 from `embeds`; tokens = LayerNorm(proj(e).view(4, 768)), one tcl_gemm_f16 and one tcl_layernorm_f16 over both."""
    from .lib import lib, stream
    L, dev = lib(), torch.device(dev)
    T, D = proj["weight"].shape[0] // proj["norm_weight"].numel(), proj["norm_weight"].numel()
    e = torch.zeros(2, proj["weight"].shape[1], dtype=H16, device=dev)
    e[1] = embeds.reshape(-1).to(dev).to(H16)
    w, b = proj["weight"].to(dev).to(H16).contiguous(), proj["bias"].to(dev).to(H16).contiguous()
    N, K = w.shape
    y = torch.empty(2, N, dtype=H16, device=dev)
    L.tcl_gemm_f16(e, w, b, 0, y, 2, N, K, K, K, N, N, 0, stream())
    out = torch.empty(2 * T, D, dtype=H16, device=dev)
    L.tcl_layernorm_f16(y, proj["norm_weight"].to(dev).to(H16).contiguous(), proj["norm_bias"].to(dev).to(H16).contiguous(), out, 2 * T, D, 1e-5, stream())
    return out.view(2, T, D)


@torch.no_grad()
def image_embeds(image_u8, encoder_path, dev, allow=False):
    """The reference image (uint8 [1, H, W, 3]) through the CLIP ViT-H/14 image tower -> image_embeds [1024] f32 on `dev`.  The engine (1.97 GB of
    f16 weights) lives only inside this call: it is freed before the UNet loop starts."""
    from . import clip
    from .model_utils import load_image_encoder_state
    state, config = load_image_encoder_state(encoder_path, allow=allow)
    engine = clip.vision_engine(state, dev, config)
    del state
    emb = engine.encode_image(image_u8)[0].clone()
    del engine
    if torch.device(dev).type == "cuda":
        torch.cuda.empty_cache()
    return emb


def make_prompt(tokens, weights, scale, dev):
    """tokens [2, T, 768] f16 and check_state's weights -> unet.ImagePrompt with the weights in f16 on `dev`."""
    from .unet import ImagePrompt
    return ImagePrompt(tokens.to(dev), {p: w.to(dev).to(H16).contiguous() for p, w in weights.items()}, scale)


def build(block, dev, allow=False):
    """hostlogic.check_ip_adapter's block {image, scale, path, image_encoder} -> unet.ImagePrompt: read on every rank, once per run."""
    proj, weights = load_state(block["path"], allow=allow)
    emb = image_embeds(read_image_u8(block["image"]), block["image_encoder"], dev, allow=allow)
    return make_prompt(image_tokens(emb, proj, dev), weights, block["scale"], dev)
