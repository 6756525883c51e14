"""init_iclight (reference: utils/model_utils.py:12-94) for the MI355X engine.

Loads the SD-1.5 UNet (HF safetensors keys), widens conv_in to 8 input channels with zero-initialised extra weights
(:21-26), ADDS the IC-Light offset file to every tensor (:47-54, strict key match), merges the LoRA of `generation.lora` on top when one is
given (generate_utils.py:95-96; tc_light_amd/lora.py), loads the VAE, and builds the SDE-DPM-Solver++ scheduler (:71-78).

A missing or mistyped weight path raises FileNotFoundError: the engine never silently relights with noise weights.  Seeded random
tensors of the same architecture (bench / tests: no network, no checkpoints in the images) must be asked for explicitly with
`models.allow_random: true` in the YAML or `TCL_ALLOW_RANDOM_WEIGHTS=1` in the environment.
"""
import json
import os
import warnings

import torch

from . import sd15
from .scheduler import DPMSolverSDEScheduler
from .unet import UNetEngine
from .vae import VAEEngine
from .vidtome import VidToMe


def allow_random(models=None):
    return bool((models or {}).get("allow_random")) or os.environ.get("TCL_ALLOW_RANDOM_WEIGHTS", "0") not in ("", "0")


def _missing(what, path, allow):
    """The one place that decides what a missing checkpoint means."""
    if not allow:
        raise FileNotFoundError(f"{what} weights not found at {path!r}. Point `models.*` of the config at the checkpoint, or opt into "
                                "seeded random stand-in weights with `models.allow_random: true` / TCL_ALLOW_RANDOM_WEIGHTS=1 "
                                "(plumbing and benchmarks only).")
    warnings.warn(f"{what} weights not found at {path!r} -> seeded random stand-ins (allow_random): outputs are not a trained model's")


def _load_safetensors(path):
    from safetensors.torch import load_file
    return load_file(path)


def _plain(raw):
    """A loaded checkpoint -> plain {name: tensor}: a `state_dict` level unwrapped and DataParallel's `module.` prefix stripped, where there is one."""
    raw = raw["state_dict"] if isinstance(raw.get("state_dict"), dict) else raw
    return {(k[7:] if k.startswith("module.") else k): v for k, v in raw.items()}


def _read_state(path):
    """A weight file (`.safetensors`, else a pickled tensor dict) -> plain {name: tensor} on the CPU, the tensors in their stored dtype."""
    return _plain(_load_safetensors(path) if path.endswith(".safetensors") else torch.load(path, map_location="cpu", weights_only=True))


def _read_config(directory):
    """The config.json dictionary of a snapshot directory, or None when it has none."""
    cfg = os.path.join(directory, "config.json")
    if os.path.isfile(cfg):
        with open(cfg) as f:
            return json.load(f)


def _with_lora(sd, lora):
    """generation.lora (generate_utils.py:95-96), merged last: the reference loads it into the pipe that already carries the offsets."""
    if lora is None:
        return sd
    from . import lora as L
    entries, weight = L.from_config(lora)
    return L.merge_into(sd, entries, weight, part="unet")


def load_unet_state(unet_path=None, offset_path=None, seed=1, allow=False, lora=None, cond_channels=4):
    """utils/model_utils.py:14-54: SD-1.5 UNet state dict with the 8-channel conv_in and the IC-Light offsets added to EVERY key; then
    `lora` (the generation.lora block or lora.LoRASet; None: nothing) merged in f32: base -> conv_in widening -> offsets -> LoRA.
    cond_channels: latent channels conv_in takes beside the 4 of x -- 4 (iclight_sd15_fc: the foreground) or 8 (iclight_sd15_fbc, :97-179
    init_iclight_bg: foreground then background, a 12-channel conv_in); the offset file must be the one of that width."""
    if cond_channels not in (4, 8):
        raise ValueError(f"cond_channels {cond_channels!r}: expected 4 (fc) or 8 (fbc)")
    cin = 4 + cond_channels
    shapes = sd15.unet_param_shapes() if cond_channels == 4 else sd15.unet_param_shapes(in_channels=cin)      # fc: the call as it always was
    if not (unet_path and os.path.exists(unet_path)):
        _missing("SD-1.5 UNet", unet_path, allow)
        return _with_lora(sd15.random_state_dict(shapes, seed), lora)
    sd = {k: v.float() for k, v in _load_safetensors(unet_path).items()}
    w = sd["conv_in.weight"]
    if w.shape[1] == 4:                                    # new_conv_in: zero weights for the concat channels (:21-26, :106-111)
        w8 = torch.zeros(w.shape[0], cin, w.shape[2], w.shape[3])
        w8[:, :4] = w
        sd["conv_in.weight"] = w8
    if not (offset_path and os.path.exists(offset_path)):
        _missing(f"IC-Light offset (iclight_sd15_{'fbc' if cond_channels == 8 else 'fc'}.safetensors)", offset_path, allow)
    else:
        off = _load_safetensors(offset_path)
        missing = [k for k in sd if k not in off]
        if missing:
            raise KeyError(f"IC-Light offset file lacks keys {missing[:3]} (reference merges strictly, model_utils.py:50-54)")
        got, want = tuple(off["conv_in.weight"].shape), tuple(sd["conv_in.weight"].shape)
        if got != want and got in ((320, 8, 3, 3), (320, 12, 3, 3)) and want in ((320, 8, 3, 3), (320, 12, 3, 3)):
            raise KeyError(f"IC-Light offset conv_in.weight is {got} (the {'fbc' if got[1] == 12 else 'fc'} model's), but generation.iclight_model "
                           f"{'fbc' if want[1] == 12 else 'fc'} takes {want}: point models.iclight_offset at that model's file")
        bad = [k for k in sd if tuple(off[k].shape) != tuple(sd[k].shape)]
        if bad:
            raise KeyError(f"IC-Light offset shape mismatch on {bad[:3]}: {tuple(off[bad[0]].shape)} vs {tuple(sd[bad[0]].shape)}")
        sd = {k: sd[k] + off[k].float() for k in sd}
    bad = [k for k, s in shapes.items() if k not in sd or tuple(sd[k].shape) != tuple(s)]
    if bad:
        raise KeyError(f"UNet checkpoint mismatch on {bad[:3]}")
    return _with_lora(sd, lora)


def load_vae_state(path=None, seed=2, allow=False):
    shapes = sd15.vae_param_shapes()
    if not (path and os.path.exists(path)):
        _missing("AutoencoderKL", path, allow)
        return sd15.random_state_dict(shapes, seed)
    raw = {k: v.float() for k, v in _load_safetensors(path).items()}
    ren = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}     # pre-0.15 diffusers VAE attention names
    sd = {}
    for k, v in raw.items():
        for a, b in ren.items():
            k = k.replace(f"attentions.0.{a}.", f"attentions.0.{b}.")
        sd[k] = v.reshape(shapes[k]) if k in shapes and v.numel() == int(torch.tensor(shapes[k]).prod()) else v
    return sd


def load_memflow_state(path=None, seed=4, allow=False):
    """MemFlowNet_things.pth (eval_utils.py:197-248: torch.load(..., weights_only=True), optional 'module.' prefix)."""
    from . import memflow
    if not (path and os.path.exists(path)):
        _missing("MemFlowNet", path, allow)
        return memflow.seeded_state_dict(memflow.memflow_param_shapes(), seed)
    return _read_state(path)


def load_raft_state(path=None, seed=5, allow=False):
    """raft-things.pth (eval_utils.py:178-195): a DataParallel state dict, keys prefixed `module.`; a plain tensor dict, so weights_only=True."""
    from . import raft
    if not (path and os.path.exists(path)):
        _missing("RAFT", path, allow)
        return raft.seeded_state_dict(seed)
    return _read_state(path)


def load_clip_state(path=None, seed=6, allow=False):
    """OpenAI CLIP weights (evaluate.py:119 clip.load("ViT-B/32")): `ViT-B-32.pt` is a TorchScript archive, so torch.jit.load(...).state_dict() is
    tried first and a plain torch.load second; a `.safetensors` file holds `transformers.CLIPModel`'s layout and goes through clip.from_hf_state."""
    from . import clip
    if not (path and os.path.exists(path)):
        _missing("CLIP", path, allow)
        return clip.seeded_state_dict(seed)
    if path.endswith(".safetensors"):
        return clip.from_hf_state(_read_state(path))
    try:
        sd = _plain(torch.jit.load(path, map_location="cpu").state_dict())
    except RuntimeError:
        sd = _read_state(path)
    return clip.from_hf_state(sd) if "visual_projection.weight" in sd else sd


def load_pick_state(path=None, seed=7, allow=False):
    """PickScore_v1 (evaluate.py:120-121 AutoModel.from_pretrained("pickapic-anonymous/PickScore_v1"), a transformers.CLIPModel at CLIP ViT-H/14) ->
    (state dict in OpenAI's key names, the config.json dictionary or None).  `path` is a snapshot directory (config.json + model.safetensors, or
    the shards model-0000x-of-0000y.safetensors with model.safetensors.index.json, or pytorch_model.bin) or a single .safetensors / .bin file.  The
    tensors keep their stored dtype and the transformers-named ones are released as they are renamed: the 3.9 GB f32 checkpoint is held once."""
    import glob
    from . import clip
    if not (path and os.path.exists(path)):
        _missing("PickScore", path, allow)
        return clip.seeded_state_dict(seed, **clip.arch_shapes(clip.PICKSCORE_V1)), None
    config, files = None, [path]
    if os.path.isdir(path):
        config = _read_config(path)
        index = os.path.join(path, "model.safetensors.index.json")
        if os.path.isfile(index):
            with open(index) as f:
                files = [os.path.join(path, n) for n in sorted(set(json.load(f)["weight_map"].values()))]
        else:
            files = [p for p in (os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")) if os.path.isfile(p)][:1] \
                or sorted(glob.glob(os.path.join(path, "model-*-of-*.safetensors")))
        absent = [p for p in files if not os.path.isfile(p)]
        if absent or not files:
            raise FileNotFoundError(f"PickScore snapshot {path!r}: " + (f"shards {absent} of its index are missing" if absent else
                                                                       "no model.safetensors, shards or pytorch_model.bin"))
    raw = {}
    for p in files:
        raw.update(_read_state(p))
    if "visual_projection.weight" not in raw:
        raise KeyError(f"{path!r} does not hold a transformers.CLIPModel (no visual_projection.weight)")
    return clip.from_hf_state(raw, consume=True), config


def load_image_encoder_state(path=None, seed=9, allow=False):
    """models.image_encoder, the CLIP ViT-H/14 image tower IP-Adapter-SD1.5 was trained on -> (the `visual.*` state dict in OpenAI's key names, the
    config.json dictionary or None).  `path` is a transformers.CLIPVisionModelWithProjection snapshot (config.json + model.safetensors or
    pytorch_model.bin) or one such file; a snapshot whose config.json is a CLIPConfig (vision_config / text_config: PickScore_v1, the same tower beside
    a text tower) goes through load_pick_state and its image half is kept."""
    from . import clip
    if not (path and os.path.exists(path)):
        _missing("CLIP ViT-H/14 image encoder", path, allow)
        shapes = {k: s for k, s in clip.clip_param_shapes(**clip.arch_shapes(clip.PICKSCORE_V1)).items() if k.startswith("visual.")}
        return clip._seeded(shapes, seed), None
    config, file = None, path
    if os.path.isdir(path):
        config = _read_config(path)
        if (config or {}).get("vision_config") is not None or os.path.isfile(os.path.join(path, "model.safetensors.index.json")):
            sd, config = load_pick_state(path)
            return clip.visual_state(sd), config
        file = next((p for p in (os.path.join(path, n) for n in ("model.safetensors", "pytorch_model.bin")) if os.path.isfile(p)), None)
        if file is None:
            raise FileNotFoundError(f"image encoder snapshot {path!r} holds neither model.safetensors nor pytorch_model.bin (models.image_encoder)")
    return clip.from_hf_vision_state(_read_state(file)), config


def load_lpips_state(vgg_path=None, lin_path=None, allow=False, seed=8):
    """The two files lpips.LPIPS(net='vgg') reads (eval_utils.py:371): `vgg_path`, a torchvision vgg16 state dict (`features.N.weight / .bias`; its
    classifier is ignored), and `lin_path`, the lpips package's weights/v0.1/vgg.pth (`lin{k}.model.1.weight`); each a .pth or a .safetensors.  ->
    one dict with both key sets, every key and shape checked (KeyError naming it) before anything is handed on.  A missing file is an error
    unless `allow`, which stands seeded tensors in for that file."""
    from . import lpips
    sd = {}
    for what, path, shapes in (("LPIPS VGG-16", vgg_path, lpips.vgg_param_shapes()), ("LPIPS linear-layer (vgg.pth)", lin_path, lpips.lin_param_shapes())):
        if not (path and os.path.exists(path)):
            _missing(what, path, allow)
            stand_in = lpips.seeded_state(seed)
            sd.update({k: stand_in[k] for k in shapes})
            continue
        raw = _read_state(path)
        for k, s in shapes.items():
            if k not in raw:
                raise KeyError(f"{what} file {path!r} lacks {k}")
            if tuple(raw[k].shape) != tuple(s):
                raise KeyError(f"{what} file {path!r}: {k} has shape {tuple(raw[k].shape)}, expected {tuple(s)}")
            sd[k] = raw[k].float()
    lpips.check_state(sd)
    return sd


def load_text_state(enc_dir):
    """The `text_encoder/` directory of an SD-1.5 snapshot (a transformers.CLIPTextModel: config.json + model.safetensors, model.fp16.safetensors or
    pytorch_model.bin, the first that exists) -> (state dict in transformers' key names with the leading `text_model.`, f32;  CLIPTextEngine's
    keyword arguments).  Read without transformers.  config.json is checked first and on the host (clip.text_options: ValueError naming the field
    for what the kernels do not cover), then against the tensors' shapes; a directory without weights is a FileNotFoundError naming it."""
    from . import clip
    config = _read_config(enc_dir)
    options, promised = clip.text_options(config)
    names = ("model.safetensors", "model.fp16.safetensors", "pytorch_model.bin")
    path = next((p for p in (os.path.join(enc_dir, n) for n in names) if os.path.isfile(p)), None)
    if path is None:
        raise FileNotFoundError(f"CLIP text encoder directory {enc_dir!r} holds none of {', '.join(names)} (models.text_encoder)")
    raw = clip.with_text_prefix(_read_state(path))
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in raw.items() if not k.endswith("embeddings.position_ids")}
    pos = sd.get("text_model.embeddings.position_embedding.weight")
    if pos is None:
        raise KeyError(f"{path!r} does not hold a transformers.CLIPTextModel (no embeddings.position_embedding.weight)")
    if config is not None:
        found = dict(width=pos.shape[1], layers=clip._layers(sd, "text_model.encoder.layers."), context_length=pos.shape[0])
        fields = dict(width="hidden_size", layers="num_hidden_layers", context_length="max_position_embeddings")
        for k, name in fields.items():
            if found[k] != promised[k]:
                raise ValueError(f"{name} {promised[k]!r} of the config.json in {enc_dir!r}, but the tensors of {path!r} say {found[k]}")
    else:                                                                  # no config.json: the head count comes from the width, OpenAI's rule
        options["heads"] = None
    return sd, options


def load_rmbg_state(path=None, seed=3, allow=False):
    """briaai/RMBG-1.4 weights (`model.safetensors` / `model.pth` with the reference module's keys, generate.py:149)."""
    from . import rmbg
    if not (path and os.path.exists(path)):
        _missing("BriaRMBG", path, allow)
        return rmbg.random_state_dict(seed)
    return _read_state(path)


def init_iclight(device="cuda", models=None, seed=12345, lora=None, cond_channels=4):
    """-> (pipe-like namespace with .unet/.vae/.scheduler, scheduler, 'iclight').  `lora`, `cond_channels`: see load_unet_state."""
    from types import SimpleNamespace
    m = models or {}
    ok = allow_random(m)
    unet = UNetEngine(load_unet_state(m.get("unet"), m.get("iclight_offset"), allow=ok, lora=lora, cond_channels=cond_channels), device,
                      VidToMe(device, seed=seed))
    vae = VAEEngine(load_vae_state(m.get("vae"), allow=ok), device)
    scheduler = DPMSolverSDEScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012)
    return SimpleNamespace(unet=unet, vae=vae, scheduler=scheduler), scheduler, "iclight"
