"""Config surface of the reference (utils/VidToMe/config_utils.py:6-74): same CLI flags, YAML keys, base_config chaining,
${a.b} interpolation and save_config -- on PyYAML instead of OmegaConf (not installed in the target image)."""
import argparse
import os
import re
from datetime import datetime

import yaml


# keys a YAML may leave out and that are not generation.* / post_opt.* settings of the Generator (those: generate.DEFAULTS)
DEFAULTS = dict(generation=dict(ip_adapter=None,                        # IP-Adapter off; else {image, scale, path} (hostlogic.check_ip_adapter)
                                detail_transfer=None,                   # detail transfer off; else {sigma, mode, blend, channels} (hostlogic.check_detail)
                                keyframes=None,                         # every frame denoised; else K or {interval, alpha, diff_threshold, eps} (check_keyframes)
                                noise_warp=None,                        # read under noise_mode warp only: {steps} (check_noise_warp)
                                fullres=None),                          # full-resolution output off; else true, a radius or {radius, eps, guide} (check_fullres)
                models=dict(ip_adapter="", image_encoder=""))           # ip-adapter_sd15.safetensors / .bin; a CLIP ViT-H/14 vision snapshot directory


class Config(dict):
    """dict with attribute access (the subset of OmegaConf the pipeline uses)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def _wrap(x):
    if isinstance(x, dict):
        return Config({k: _wrap(v) for k, v in x.items()})
    if isinstance(x, list):
        return [_wrap(v) for v in x]
    return x


def _merge(base, over):
    out = Config(base)
    for k, v in over.items():
        out[k] = _merge(base[k], v) if isinstance(v, dict) and isinstance(base.get(k), dict) else v
    return out


def _resolve(cfg, root=None):
    root = cfg if root is None else root

    def look(path):
        cur = root
        for p in path.split("."):
            cur = cur[p]
        return _sub(cur) if isinstance(cur, str) else cur

    def _sub(s):
        m = re.fullmatch(r"\$\{([\w.]+)\}", s)
        if m:
            return look(m.group(1))
        return re.sub(r"\$\{([\w.]+)\}", lambda mm: str(look(mm.group(1))), s)
    for k, v in list(cfg.items()):
        if isinstance(v, dict):
            _resolve(v, root)
        elif isinstance(v, str) and "${" in v:
            cfg[k] = _sub(v)
    return cfg


def load_yaml_chain(path, base_override=None):
    cfg = _wrap(yaml.safe_load(open(path)))
    cur, cur_path = cfg, path
    if base_override is not None:
        cur["base_config"] = base_override
    while "base_config" in cur and cur["base_config"] != cur_path:
        base = _wrap(yaml.safe_load(open(cur["base_config"])))
        cfg = _merge(base, cfg)
        cur_path, cur = cur["base_config"], base
    return cfg


def load_config(argv=None, print_config=True):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="configs/tclight_default.yaml", help="Config file path")
    ap.add_argument("--base_config", type=str, default=None, help="Base config file path to override")
    ap.add_argument("--input_path", "-i", type=str, default=None, help="path to video, for a fast usage")
    ap.add_argument("--prompt", "-p", type=str, default=None, help="prompt for video relighting, for a fast usage")
    ap.add_argument("--negative_prompt", "-n", type=str, default=None, help="negative prompt, for a fast usage")
    ap.add_argument("--multi_axis", action="store_true", help="use multi-axis denoising, for a fast usage")
    # not in the reference's run.py: IC-Light's own "Lighting Preference" (generation.init_latent / init_strength, generate.py DEFAULTS)
    ap.add_argument("--light", choices=("left", "right", "top", "bottom", "source"), default=None,
                    help="start the denoise from a light gradient of that side (or the source frames), for a fast usage")
    ap.add_argument("--strength", type=float, default=None, help="how far the relight may move from that start, in (0, 1], for a fast usage")
    # IC-Light's highres pass (generation.highres_scale / highres_denoise, generate.py DEFAULTS)
    ap.add_argument("--highres_scale", type=float, default=None, help="resize the relit frames by this factor in [1, 3] (to multiples of 64) and "
                    "refine them with a second denoise; 1.0 is off, for a fast usage")
    ap.add_argument("--highres_denoise", type=float, default=None, help="strength of that second denoise, in (0, 1], for a fast usage")
    # IC-Light's background-conditioned model (generation.iclight_model / bg_source, generate.py DEFAULTS)
    ap.add_argument("--iclight_model", choices=("fc", "fbc"), default=None, help="fc: the foreground-conditioned model; fbc: foreground and "
                    "background, the background is the lighting condition (models.iclight_offset must be that model's file), for a fast usage")
    ap.add_argument("--bg_source", choices=("upload", "upload_flip", "left", "right", "top", "bottom", "grey"), default=None,
                    help="the background of the fbc model: generation.background_image_path (as it is or flipped), a grey ramp or flat grey, "
                    "for a fast usage")
    # IC-Light's "Compute Normal" on the fbc model (generation.normal, generate.py DEFAULTS)
    ap.add_argument("--normal", action="store_true", help="fbc only: relight under the left / right / bottom / top ramps with one seed and write "
                    "per-frame normal maps and the ambient video instead of one relight, for a fast usage")
    # an animated light (generation.light_path, generate.py DEFAULTS)
    ap.add_argument("--light_sweep", type=float, nargs=2, metavar=("A0", "A1"), default=None,
                    help="turn the light from angle A0 at the first frame to A1 at the last (degrees, the side it comes FROM: 0 left, 90 top, "
                    "180 right, 270 bottom): generation.light_path [[0, A0], [1, A1]], for a fast usage")
    # a prompt that changes over the clip (generation.prompt_path, generate.py DEFAULTS)
    ap.add_argument("--prompt_sweep", type=str, nargs=2, metavar=("PROMPT_A", "PROMPT_B"), default=None,
                    help="blend the text conditioning from PROMPT_A at the first frame to PROMPT_B at the last: generation.prompt_path "
                    "[[0, PROMPT_A], [1, PROMPT_B]]; -p / generation.prompt still names the run, for a fast usage")
    # IP-Adapter: relight towards a reference image (generation.ip_adapter, generate.py DEFAULTS)
    ap.add_argument("--ip_image", type=str, default=None, help="a reference image the relight is steered towards through IP-Adapter "
                    "(models.ip_adapter, models.image_encoder): generation.ip_adapter.image, for a fast usage")
    ap.add_argument("--ip_scale", type=float, default=None, help="weight of the image attention in [0, 2] (generation.ip_adapter.scale), for a fast usage")
    # detail transfer: the source's high frequencies back onto the relit frames (generation.detail_transfer, generate.py DEFAULTS)
    ap.add_argument("--detail", type=float, nargs="?", const=3.0, default=None, metavar="SIGMA",
                    help="give the relit frames the source's detail back, the blur's sigma in [0.5, 16] (3 when left out): "
                    "generation.detail_transfer.sigma, for a fast usage")
    ap.add_argument("--detail_mode", choices=("add", "ratio"), default=None, help="add: the source's high-pass is added; ratio: the source times the "
                    "ratio of the two blurs (generation.detail_transfer.mode), for a fast usage")
    ap.add_argument("--detail_blend", type=float, default=None, help="strength of the step in [0, 1] (generation.detail_transfer.blend), for a fast usage")
    # keyframe relighting: only every K-th frame is denoised, the others are propagated along the flows (generation.keyframes, generate.py DEFAULTS)
    ap.add_argument("--keyframes", type=int, default=None, metavar="K", help="denoise only every K-th frame (K in [1, 16]) and carry the relight to "
                    "the frames in between along the optical flow: generation.keyframes.interval, for a fast usage")
    # the noise of the clip (generation.noise_mode / noise_warp, generate.py DEFAULTS)
    ap.add_argument("--noise_mode", type=str, default=None, help="same: one noise frame for the whole clip; vanilla: independent noise per frame; "
                    "warp: the noise is carried from frame to frame along the optical flow (generation.noise_mode), for a fast usage")
    ap.add_argument("--noise_warp_steps", type=int, choices=(0, 1), default=None, help="under --noise_mode warp: 1 (default) warps the per-step "
                    "noise of the SDE solver too, 0 draws it per frame as before (generation.noise_warp.steps), for a fast usage")
    # full-resolution output: the relight applied to the source's own pixels (generation.fullres, generate.py DEFAULTS)
    ap.add_argument("--fullres", type=int, nargs="?", const=8, default=None, metavar="RADIUS",
                    help="write output_fullres.* at the source's own resolution: a guided-filter fit of relit ~ a * source + b at the working size, "
                    "radius in [1, 64] (8 when left out), applied to the native frames: generation.fullres.radius, for a fast usage")
    ap.add_argument("--fullres_eps", type=float, default=None, help="the fit's regulariser in [1e-4, 1] (generation.fullres.eps), for a fast usage")
    ap.add_argument("--fullres_guide", choices=("rgb", "luma"), default=None, help="rgb: every channel guided by itself; luma: the source's "
                    "luminance guides all three (generation.fullres.guide), for a fast usage")
    a = ap.parse_args(argv)
    cfg = load_yaml_chain(a.config, a.base_config)
    if a.fullres is not None or a.fullres_eps is not None or a.fullres_guide is not None:
        block = cfg.generation.get("fullres")
        block = Config(dict(radius=block) if isinstance(block, int) and not isinstance(block, bool) else (block if isinstance(block, dict) else {}))
        for key, v in (("radius", a.fullres), ("eps", a.fullres_eps), ("guide", a.fullres_guide)):
            if v is not None:
                block[key] = v
        cfg.generation.fullres = block
    if a.noise_mode is not None:
        cfg.generation.noise_mode = a.noise_mode
    if a.noise_warp_steps is not None:
        block = cfg.generation.get("noise_warp")
        cfg.generation.noise_warp = Config(dict(block if isinstance(block, dict) else {}, steps=bool(a.noise_warp_steps)))
    if a.keyframes is not None:
        block = cfg.generation.get("keyframes")
        cfg.generation.keyframes = Config(dict(block, interval=a.keyframes)) if isinstance(block, dict) else a.keyframes
    if a.ip_image is not None or a.ip_scale is not None:
        block = Config(cfg.generation.get("ip_adapter") or {})
        if a.ip_image is not None:
            block["image"] = a.ip_image
        if a.ip_scale is not None:
            block["scale"] = a.ip_scale
        cfg.generation.ip_adapter = block
    if a.detail is not None or a.detail_mode is not None or a.detail_blend is not None:
        block = cfg.generation.get("detail_transfer")
        block = Config(dict(sigma=block) if isinstance(block, (int, float)) and not isinstance(block, bool) else (block or {}))
        for key, v in (("sigma", a.detail), ("mode", a.detail_mode), ("blend", a.detail_blend)):
            if v is not None:
                block[key] = v
        cfg.generation.detail_transfer = block
    if a.prompt_sweep is not None:
        cfg.generation.prompt_path = [[0.0, a.prompt_sweep[0]], [1.0, a.prompt_sweep[1]]]
    if a.light_sweep is not None:
        cfg.generation.light_path = [[0.0, float(a.light_sweep[0])], [1.0, float(a.light_sweep[1])]]
    if a.normal:
        cfg.generation.normal = True
    if a.iclight_model is not None:
        cfg.generation.iclight_model = a.iclight_model
    if a.bg_source is not None:
        cfg.generation.bg_source = a.bg_source
    if a.highres_scale is not None:
        cfg.generation.highres_scale = a.highres_scale
    if a.highres_denoise is not None:
        cfg.generation.highres_denoise = a.highres_denoise
    if a.light is not None:
        cfg.generation.init_latent = a.light
    if a.strength is not None:
        cfg.generation.init_strength = a.strength
    if a.input_path is not None and cfg.data.scene_type.lower() == "video":
        cfg.data.rgb_path = a.input_path
    if a.multi_axis:
        cfg.generation.alpha_t = 0.01
    if a.negative_prompt is not None:
        cfg.generation.negative_prompt = a.negative_prompt
    if a.prompt is not None or isinstance(cfg.generation.prompt, str):
        prompt = cfg.generation.prompt if a.prompt is None else a.prompt
        # the reference names the run after data.rgb_path; a scene without one (sceneflow) is named after its scene_path
        src = cfg.data.get("rgb_path") or str(cfg.data.get("scene_path", cfg.data.scene_type)).replace("/", "_")
        video = os.path.splitext(os.path.basename(src))[0]
        cfg.work_dir = os.path.join(cfg.work_dir, datetime.now().strftime("%m-%d-%Y"), video)
        os.makedirs(cfg.work_dir, exist_ok=True)
        prev = [int(x[-5:]) for x in os.listdir(cfg.work_dir) if x[-5:].isdigit()]
        cfg.generation.prompt = Config({f"{prompt}-{str(max(prev) + 1 if prev else 0).zfill(5)}": prompt})
    if isinstance(cfg.generation.prompt, str):
        cfg.generation.prompt = Config({"edit": cfg.generation.prompt})
    _resolve(cfg)
    if print_config:
        print("[INFO] loaded config:")
        print(yaml.safe_dump(_plain(cfg), sort_keys=False))
    return cfg


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def save_config(config, path, gene=False, inv=False):
    os.makedirs(path, exist_ok=True)
    c = _plain(config)
    if gene:
        c.pop("inversion", None)
    if inv:
        c.pop("generation", None)
    with open(os.path.join(path, "config.yaml"), "w") as f:
        yaml.safe_dump(c, f, sort_keys=False)
