"""`generation.use_lora` / `generation.lora` (reference: utils/VidToMe/generate_utils.py:95-96, `pipe.load_lora_weights(**gene_config.lora)`).

The reference hangs the adapter on the pipe and pays `up(down(x))` in every forward; here the single adapter is MERGED into the weights once,
on the host, before the engine packs them:  W += weight * (alpha / r) * up @ down  -- the UNet engine then runs its usual kernels on other numbers.

Two file layouts are read (the key rules are written from the formats):
  kohya             lora_unet_<module path, '.' -> '_'>.lora_down.weight / .lora_up.weight / .alpha      (lora_te_<...> for the text encoder)
  diffusers / PEFT  unet.<module path>.lora_A.weight / .lora_B.weight [/ .alpha]                        (text_encoder.<...>)
                    and the older spellings  <path>.lora.down.weight / .lora.up.weight  and
                    <attn>.processor.to_q_lora.down.weight / .up.weight  (to_k_lora, to_v_lora, to_out_lora -> to_out.0; in the text encoder
                    q_proj, k_proj, v_proj, out_proj).
Every entry is normalised to `(target_key, down, up, alpha_or_None)` with the kohya module name as `target_key` (`lora_unet_...` /
`lora_te_...`): that is the one spelling both layouts reach without knowing the model.  Its underscores are ambiguous (`to_out_0` vs
`to_out.0`), so `merge_into` resolves them against the keys of the state dict it is given.  Strict like the IC-Light offset merge: an entry
of the merged part that maps to no tensor is a `KeyError` naming the first three, a shape that does not fit a `ValueError`.
"""
import os
import re
from collections import namedtuple

import torch

LoRASet = namedtuple("LoRASet", "entries weight")          # what from_config returns: the normalised entries and generation.lora.lora_weight

_PART = {"unet": "lora_unet_", "te": "lora_te_"}
_PEFT_ROOT = {"unet": "lora_unet_", "text_encoder": "lora_te_"}
_OLD_ATTN = {"to_q_lora": "to_q", "to_k_lora": "to_k", "to_v_lora": "to_v", "to_out_lora": "to_out.0"}
_OLD_ATTN_TE = {"to_q_lora": "q_proj", "to_k_lora": "k_proj", "to_v_lora": "v_proj", "to_out_lora": "out_proj"}
# suffix -> slot; the first that matches wins
_SUFFIX = ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".lora_A.weight", "down"), (".lora_B.weight", "up"),
           (".lora.down.weight", "down"), (".lora.up.weight", "up"), (".down.weight", "down"), (".up.weight", "up"), (".alpha", "alpha"))


def _split(key):
    """file key -> (target_key, slot) or None when the key belongs to neither layout."""
    for suf, slot in _SUFFIX:
        if key.endswith(suf):
            mod = key[:-len(suf)]
            break
    else:
        return None
    if mod.startswith(("lora_unet_", "lora_te_")):                                       # kohya: already the normal form
        return (mod, slot) if "." not in mod else None
    root, _, path = mod.partition(".")
    if root not in _PEFT_ROOT or not path:
        return None
    old = _OLD_ATTN if root == "unet" else _OLD_ATTN_TE
    parts = [old.get(p, p) for p in path.split(".") if p != "processor"]
    if any(p.endswith("_lora") for p in parts):
        return None
    return _PEFT_ROOT[root] + ".".join(parts).replace(".", "_"), slot


def _read(path_or_dict, weight_name=None):
    if isinstance(path_or_dict, dict):
        return path_or_dict
    path = os.fspath(path_or_dict)
    if os.path.isdir(path):
        if not weight_name:
            raise FileNotFoundError(f"LoRA: {path!r} is a directory; name the file in it with generation.lora.lora_weight_name")
        path = os.path.join(path, weight_name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"LoRA weights not found at {path!r} (generation.lora.pretrained_model_name_or_path_or_dict / lora_weight_name; "
                                "a hub id cannot be fetched: give a local .safetensors file)")
    if not path.endswith(".safetensors"):
        raise ValueError(f"LoRA file {path!r}: only .safetensors files are read")
    from safetensors.torch import load_file
    return load_file(path)


def load_lora(path_or_dict, weight_name=None):
    """A `.safetensors` file, a directory plus `weight_name`, or an in-memory dict, in either layout ->
    [(target_key, down, up, alpha_or_None)] sorted by target_key; down / up keep their stored dtype and shape, alpha is a float."""
    raw = _read(path_or_dict, weight_name)
    mods, unknown = {}, []
    for k, v in raw.items():
        hit = _split(k)
        if hit is None:
            unknown.append(k)
            continue
        slot = mods.setdefault(hit[0], {})
        if hit[1] in slot:
            raise ValueError(f"LoRA: {hit[0]} has two '{hit[1]}' tensors (one of them under {k!r})")
        slot[hit[1]] = v
    if unknown:
        raise KeyError(f"LoRA: keys of neither the kohya nor the diffusers / PEFT layout: {sorted(unknown)[:3]}")
    half = sorted(m for m, s in mods.items() if "down" not in s or "up" not in s)
    if half:
        raise ValueError(f"LoRA: entries without both a down and an up matrix: {half[:3]}")
    if not mods:
        raise ValueError("LoRA: the file holds no tensors")
    return [(m, s["down"], s["up"], float(s["alpha"]) if "alpha" in s else None) for m, s in sorted(mods.items())]


def from_config(block):
    """The `generation.lora` block (the reference's `load_lora_weights` keywords) -> LoRASet(entries, weight).  Raises before anything
    else is loaded: no block / no path is a ValueError, a missing file a FileNotFoundError.  `lora_adapter` is accepted and ignored:
    there is a single adapter and it is merged."""
    if isinstance(block, LoRASet):
        return block
    if not block:
        raise ValueError("generation.use_lora is true but there is no generation.lora block (pretrained_model_name_or_path_or_dict, "
                         "lora_weight_name, lora_weight)")
    src = block.get("pretrained_model_name_or_path_or_dict")
    if src is None or (isinstance(src, str) and not src):
        raise ValueError("generation.lora.pretrained_model_name_or_path_or_dict is empty: name the LoRA's .safetensors file or its directory")
    w = block.get("lora_weight")
    return LoRASet(load_lora(src, block.get("lora_weight_name")), 1.0 if w is None else float(w))


def has_part(entries, part):
    return any(e[0].startswith(_PART[part]) for e in entries)


def _resolve(sd, entries, part):
    """kohya module names of `part` -> the `<module>.weight` key of `sd` they spell with '.' for some of the '_'."""
    table = {}
    for k in sd:
        if k.endswith(".weight"):
            flat = k[:-len(".weight")].replace(".", "_")
            if flat in table:
                raise ValueError(f"LoRA: {table[flat]!r} and {k!r} spell the same kohya name; the state dict cannot be addressed")
            table[flat] = k
    mine = [e for e in entries if e[0].startswith(_PART[part])]
    lost = [e[0] for e in mine if e[0][len(_PART[part]):] not in table]
    if lost:
        raise KeyError(f"LoRA targets that map to no {part} tensor: {lost[:3]}" + (f" (+{len(lost) - 3} more)" if len(lost) > 3 else ""))
    return [(table[e[0][len(_PART[part]):]], e) for e in mine]


def _delta(name, W, down, up):
    """up @ down in f32, shaped like W (or like W's first 4 input channels for a 4-channel conv_in LoRA)."""
    if down.dim() not in (2, 4) or up.dim() != down.dim():
        raise ValueError(f"LoRA {name}: down {tuple(down.shape)} / up {tuple(up.shape)} are not a linear or convolution pair")
    r = down.shape[0]
    if up.shape[1] != r or any(s != 1 for s in up.shape[2:]):
        raise ValueError(f"LoRA {name}: up {tuple(up.shape)} does not contract with down {tuple(down.shape)} over the rank {r}")
    want = tuple(W.shape)
    if W.dim() == 4 and down.dim() == 2:                       # a linear pair on a 1x1 convolution (proj_in / proj_out)
        got = (up.shape[0], down.shape[1], 1, 1)
    elif W.dim() == 2 and down.dim() == 4:                     # a 1x1 convolution pair on a linear layer
        got = (up.shape[0], down.shape[1]) if tuple(down.shape[2:]) == (1, 1) else None
    else:
        got = (up.shape[0],) + tuple(down.shape[1:])
    narrow = name == "conv_in.weight" and got == (want[0], 4) + want[2:] and want[1] in (8, 12)
    if got != want and not narrow:
        raise ValueError(f"LoRA {name}: up @ down gives {got if got else tuple(down.shape)}, the weight is {want}")
    d = up.float().flatten(1) @ down.float().flatten(1)        # [out, r] @ [r, in * kh * kw]
    return d.reshape(got), narrow


def merge_into(sd, entries, weight=1.0, part="unet"):
    """W += weight * (alpha / r) * up @ down (alpha = r when absent) for every entry of `part` ("unet": lora_unet_*, "te": lora_te_*), in f32
    on the host; entries of the other part are left to the other state dict.  Linear: [out, r] @ [r, in]; 1x1 convolutions the same on the
    squeezed kernel; 3x3 (LoCon): down [r, in, 3, 3], up [out, r, 1, 1], contracted over r.  A conv_in LoRA with 4 input channels goes to
    the first 4 input channels of the 8-channel (fc) or 12-channel (fbc) IC-Light conv_in.  Everything is checked before anything is written; the merged tensors
    replace their entries in `sd` (f32), which is returned.  weight == 0 leaves `sd` untouched."""
    todo = []
    for key, (name, down, up, alpha) in _resolve(sd, entries, part):
        d, narrow = _delta(key, sd[key], down, up)
        r = down.shape[0]
        todo.append((key, d, float(weight) * ((r if alpha is None else alpha) / r), narrow))
    if float(weight) == 0.0:
        return sd
    for key, d, scale, narrow in todo:
        W = sd[key].float().clone()
        if narrow:
            W[:, :4] += scale * d
        else:
            W += scale * d
        sd[key] = W
    return sd
