"""Integer host logic of the denoising loop: chunking, yt-plane windows, decay schedule (no tensors on the data path).

get_chunks        utils/VidToMe/generate_utils.py:174-205
temporal_windows  generate.py:246-260
alpha_schedule    generate.py:228-229
The reference draws from the global numpy / torch CPU RNGs; here the draws come from explicit seeded streams so that
"identical seeds" means the same choices on any device (hard part 3).
"""
import math

import numpy as np
import torch


def chunks_from_draws(flen, chunk_size, rand_first, flip_draw, perm, merge_global=True, chunk_ord="mix", perm_div=4.0):
    """Pure function of the three draws: rand_first in [0, chunk_size), flip_draw in [0,1), perm = permutation of chunk ids."""
    first = rand_first + 1
    bounds = [(0, min(first, flen))]
    s = first
    while s < flen:
        bounds.append((s, min(s + chunk_size, flen)))
        s += chunk_size
    chunks = [list(range(a, b)) for a, b in bounds]
    if flip_draw > 0.5:
        chunks = chunks[::-1]
    if not merge_global:
        return chunks
    order = [int(p) for p in perm] if chunk_ord in ("rand", "mix") else list(range(len(chunks)))
    if chunk_ord == "mix":
        # the first len/perm_div draws stay in drawn order; the remaining chunks follow in index order, walked from whichever end lies
        # nearer (in chunk index) to the last drawn one (generate_utils.py:189-201)
        head = order[:int(len(order) / perm_div)]
        tail = sorted(order[len(head):])
        if head and tail and abs(tail[-1] - head[-1]) < abs(tail[0] - head[-1]):
            tail.reverse()
        order = head + tail
    return [chunks[i] for i in order]


def n_chunks(flen, chunk_size, rand_first):
    first = rand_first + 1
    return 1 + max(0, math.ceil((flen - first) / chunk_size))


class ChunkSampler:
    """Seeded stand-in for the np.random / torch.randperm calls of get_chunks."""

    def __init__(self, seed, chunk_size=4, merge_global=True, chunk_ord="mix-4"):
        self.np_rng = np.random.RandomState(seed)
        self.t_gen = torch.Generator(device="cpu").manual_seed(int(seed))
        self.chunk_size, self.merge_global = chunk_size, merge_global
        self.perm_div = float(chunk_ord.split("-")[-1]) if "-" in chunk_ord else 3.0
        self.chunk_ord = "mix" if "mix" in chunk_ord else chunk_ord

    def get_chunks(self, flen):
        rf = int(self.np_rng.randint(0, self.chunk_size))
        fl = float(self.np_rng.rand())
        n = n_chunks(flen, self.chunk_size, rf)
        perm = torch.randperm(n, generator=self.t_gen) if (self.merge_global and self.chunk_ord in ("rand", "mix")) else torch.arange(n)
        return chunks_from_draws(flen, self.chunk_size, rf, fl, perm, self.merge_global, self.chunk_ord, self.perm_div)


def temporal_windows(n, win):
    """-> (window starts, overlaps): n_slices = ceil((n-1)/(win-1)); later windows overwrite then scale the overlap."""
    n_slices = math.ceil((n - 1) / (win - 1)) if n > 1 else 1
    if n_slices > 1:
        total = n_slices * win - n
        ov = total // (n_slices - 1)
        last = ov + total % (n_slices - 1)
        ovl = [ov] * (n_slices - 2) + [last]
        cs = np.cumsum(ovl)
        return [0] + [int((i + 1) * win - cs[i]) for i in range(n_slices - 1)], [int(o) for o in ovl]
    return [0], [0]


def alpha_schedule(alpha_t, final_factor_t, n_steps):
    return [alpha_t * final_factor_t ** min(i / n_steps, 1) for i in range(n_steps)]


INIT_LATENTS = ("none", "left", "right", "top", "bottom", "source")       # generation.init_latent; the four sides in the order of TCL_LIGHT_*


def check_init(init_latent, init_strength, n_timesteps=None):
    """generation.init_latent / init_strength as (str, float); anything else is a ValueError (run.py raises it before a model is loaded).
    With n_timesteps: a schedule that would execute no step at all is refused too (diffusers' img2img pipeline does the same)."""
    name = "none" if init_latent is None else str(init_latent).lower()
    if name not in INIT_LATENTS:
        raise ValueError(f"generation.init_latent {init_latent!r}: expected one of {' | '.join(INIT_LATENTS)}")
    if isinstance(init_strength, bool) or not isinstance(init_strength, (int, float)) or not 0.0 < float(init_strength) <= 1.0:
        raise ValueError(f"generation.init_strength {init_strength!r}: expected a number in (0, 1]")
    if n_timesteps is not None and name != "none" and img2img_schedule(n_timesteps, init_strength)[2] < 1:
        raise ValueError(f"generation.init_strength {init_strength} with n_timesteps {n_timesteps} leaves no step to execute")
    return name, float(init_strength)


def img2img_schedule(n, strength):
    """-> (scheduler steps, begin index, steps executed) of an img2img start (gradio_demo_iclight.py:293 and diffusers' img2img get_timesteps,
    restated): the scheduler is set to round(n / strength) steps and the loop runs the last int(steps * strength) of them -- n, give or take one."""
    n_sched = int(round(n / strength))
    run = min(int(n_sched * strength), n_sched)
    return n_sched, n_sched - run, run


def highres_size(H, W, scale):
    """(H2, W2) of the highres pass (gradio_demo_iclight.py:310-312): every side goes to int(round(side * scale / 64.0)) * 64 with Python's round
    (half to even: 960 * 1.5 -> 1408, not 1472); a side below 64 is a ValueError."""
    out = tuple(int(round(int(s) * float(scale) / 64.0)) * 64 for s in (H, W))
    if min(out) < 64:
        raise ValueError(f"generation.highres_scale {scale} takes {int(H)}x{int(W)} to {out[0]}x{out[1]}: a side below 64")
    return out


def check_highres(highres_scale, highres_denoise, n_timesteps=None, background_cond=False):
    """generation.highres_scale / highres_denoise as (float, float); anything else is a ValueError (run.py raises it before a model is loaded).
    scale in [1, 3], 1.0 = off; denoise in (0, 1].  With the pass on: a schedule that would execute no step is refused (as check_init does), and so
    is background compositing (generation.background_cond), which the highres pass does not cover."""
    for key, v in (("highres_scale", highres_scale), ("highres_denoise", highres_denoise)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"generation.{key} {v!r}: expected a number")
    scale, denoise = float(highres_scale), float(highres_denoise)
    if not 1.0 <= scale <= 3.0:
        raise ValueError(f"generation.highres_scale {highres_scale!r}: expected a number in [1, 3] (1.0 = off)")
    if not 0.0 < denoise <= 1.0:
        raise ValueError(f"generation.highres_denoise {highres_denoise!r}: expected a number in (0, 1]")
    if scale != 1.0:
        if n_timesteps is not None and img2img_schedule(n_timesteps, denoise)[2] < 1:
            raise ValueError(f"generation.highres_denoise {highres_denoise} with n_timesteps {n_timesteps} leaves no step to execute")
        if background_cond:
            raise ValueError("generation.background_cond together with generation.highres_scale > 1 is not supported: the highres pass does not "
                             "composite backgrounds")
    return scale, denoise


ICLIGHT_MODELS = ("fc", "fbc")            # generation.iclight_model: foreground-conditioned (8-channel conv_in) | foreground + background (12)
BG_SOURCES = ("upload", "upload_flip", "left", "right", "top", "bottom", "grey")       # generation.bg_source (fbc only)
# bg_source -> (TCL_LIGHT_* side naming the axis, first sample, last sample) of uint8(np.linspace(first, last, n)): IC-Light's background demo
BG_RAMPS = {"left": (0, 224, 32), "right": (1, 32, 224), "top": (2, 224, 32), "bottom": (3, 32, 224), "grey": (0, 64, 64)}


def cond_channels(iclight_model):
    """Latent channels conv_in takes beside the 4 of x: 4 (fc: the foreground) or 8 (fbc: foreground, then background)."""
    return 8 if iclight_model == "fbc" else 4


def check_fbc(iclight_model, bg_source, init_latent="none", highres_scale=1.0, background_cond=False, inversion=False):
    """generation.iclight_model / bg_source as (str, str); anything else is a ValueError (run.py, invert.py and Generator raise it before a model
    is loaded).  Under fbc the background is the lighting condition, so what this engine has not built for it is refused by name: an img2img
    start (init_latent), the highres pass, background compositing (background_cond) and DDIM inversion."""
    model = "fc" if iclight_model is None else str(iclight_model).lower()
    if model not in ICLIGHT_MODELS:
        raise ValueError(f"generation.iclight_model {iclight_model!r}: expected one of {' | '.join(ICLIGHT_MODELS)}")
    source = "upload" if bg_source is None else str(bg_source).lower()
    if source not in BG_SOURCES:
        raise ValueError(f"generation.bg_source {bg_source!r}: expected one of {' | '.join(BG_SOURCES)}")
    if model == "fbc":
        if inversion:
            raise ValueError("generation.iclight_model fbc: DDIM inversion (invert.py) is not supported for the background-conditioned model")
        if init_latent is not None and str(init_latent).lower() != "none":
            raise ValueError(f"generation.iclight_model fbc together with generation.init_latent {init_latent!r} is not supported: the background "
                             "is the lighting condition")
        if isinstance(highres_scale, bool) or not isinstance(highres_scale, (int, float)) or float(highres_scale) != 1.0:
            raise ValueError(f"generation.iclight_model fbc together with generation.highres_scale {highres_scale!r} is not supported")
        if background_cond:
            raise ValueError("generation.iclight_model fbc together with generation.background_cond is not supported: fbc takes the background "
                             "as a condition (generation.bg_source) instead of compositing it")
    return model, source


def fbc_background_per_frame(n_background, n_frames, bg_source="upload"):
    """The uploaded background of the fbc model is one frame for all (-> False) or exactly one per frame of the run (-> True; with a single frame:
    False); any other length is a ValueError.  The answer depends on the run's totals only, so every rank gives the same one."""
    if n_background not in (1, n_frames):
        raise ValueError(f"generation.background_image_path yields {n_background} frames: generation.bg_source {bg_source} takes 1 or "
                         f"exactly {n_frames} (the frames of this run)")
    return n_background == n_frames and n_frames > 1


NORMAL_SIDES = ("left", "right", "bottom", "top")        # generation.normal: the four relights, in the order process_normal runs them
NORMAL_MATTE_SIGMA = 16.0                                # process_normal's run_rmbg(input_fg, sigma=16)


def check_normal(normal, iclight_model="fc", fbc_matting=True, apply_opt=True):
    """generation.normal (IC-Light's "Compute Normal", the background demo's process_normal): false -> (), nothing else is looked at.  true -> the
    bg_source ramps of the four relights in the demo's order.  It needs the background-conditioned model, so normal under iclight_model fc is a
    ValueError naming both keys; normal and fbc_matting must be booleans.  apply_opt may be either: Generator.normals never runs stage 1 / 2
    (exposure alignment per direction would bias the ratios), run.py says so and records apply_opt: false."""
    if normal is None:
        normal = False
    if not isinstance(normal, bool):
        raise ValueError(f"generation.normal {normal!r}: expected true or false")
    if not normal:
        return ()
    model = "fc" if iclight_model is None else str(iclight_model).lower()
    if model != "fbc":
        raise ValueError(f"generation.normal needs generation.iclight_model fbc (got {iclight_model!r}): the normal is computed from four relights "
                         "of the background-conditioned model")
    if not isinstance(fbc_matting, bool):
        raise ValueError(f"generation.normal: generation.fbc_matting {fbc_matting!r}: expected true or false")
    if not isinstance(apply_opt, bool):
        raise ValueError(f"generation.normal: post_opt.apply_opt {apply_opt!r}: expected true or false")
    return NORMAL_SIDES


LIGHT_AXIS_SIDES = ("left", "top", "right", "bottom")     # reduced angle 0 / 90 / 180 / 270: the side the light comes FROM
LIGHT_AXIS_DIRS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
# iclight_model -> (hi, lo) levels of the animated ramps: those of tcl_light_gradient_f32 (fc) and of the bg_source ramps (fbc, BG_RAMPS)
LIGHT_LEVELS = {"fc": (255, 0), "fbc": (224, 32)}


def _is_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float))


def check_light_path(path, init_latent="none", normal=False, iclight_model="fc", bg_source=None, init_strength=None, n_timesteps=None):
    """generation.light_path: None (off: nothing else is looked at) or keyframes [[pos, angle_deg], ...] -> [[float, float], ...]; anything else is a
    ValueError (run.py and Generator raise it before a model is loaded).  pos in [0, 1], non-decreasing, the first 0 and the last 1 -- a single
    keyframe [[0, a]] is a constant direction; angle_deg any finite number, the side the light comes FROM (0 left, 90 top, 180 right, 270 bottom),
    beyond 360 allowed (several turns).  Refused by both key names: init_latent other than none (the path is the start), normal (the four ramps are
    the lights), and under fbc a bg_source other than the default upload (the per-frame ramps are the backgrounds).  Under fc the start is an img2img
    one, so with init_strength and n_timesteps a schedule that would execute no step is refused as check_init refuses it."""
    if path is None:
        return None
    if not isinstance(path, (list, tuple)) or len(path) == 0:
        raise ValueError(f"generation.light_path {path!r}: expected null or a list of keyframes [[pos, angle_deg], ...] with at least one")
    keys = []
    for kf in path:
        if not isinstance(kf, (list, tuple)) or len(kf) != 2 or not all(_is_number(v) and math.isfinite(v) for v in kf):
            raise ValueError(f"generation.light_path keyframe {kf!r}: expected [pos, angle_deg], two finite numbers")
        keys.append([float(kf[0]), float(kf[1])])
    pos = [k[0] for k in keys]
    if pos[0] != 0.0 or (len(keys) > 1 and pos[-1] != 1.0) or any(b < a for a, b in zip(pos, pos[1:])) or not all(0.0 <= p <= 1.0 for p in pos):
        raise ValueError(f"generation.light_path positions {pos}: expected non-decreasing values in [0, 1], the first 0 and (with more than one "
                         "keyframe) the last 1")
    if init_latent is not None and str(init_latent).lower() != "none":
        raise ValueError(f"generation.light_path together with generation.init_latent {init_latent!r} is not supported: the path is the start")
    if normal:
        raise ValueError("generation.light_path together with generation.normal is not supported: the normal is computed from the four fixed ramps")
    model = "fc" if iclight_model is None else str(iclight_model).lower()
    if model == "fbc" and bg_source is not None and str(bg_source).lower() != "upload":
        raise ValueError(f"generation.light_path together with generation.bg_source {bg_source!r} is not supported under iclight_model fbc: the "
                         "per-frame ramps are the backgrounds, leave bg_source at its default")
    if model != "fbc" and init_strength is not None and n_timesteps is not None and img2img_schedule(n_timesteps, init_strength)[2] < 1:
        raise ValueError(f"generation.light_path: generation.init_strength {init_strength} with n_timesteps {n_timesteps} leaves no step to execute")
    return keys


def light_positions(n_total, lo=0, hi=None):
    """pos = i/(N - 1) of the run's frames lo <= i < hi (GLOBAL indices: a rank of a sharded run builds what one rank would); N == 1 -> 0."""
    hi = n_total if hi is None else hi
    return [i / (n_total - 1) if n_total > 1 else 0.0 for i in range(lo, hi)]


def light_angles(path, positions):
    """The angle (degrees, f64) at every position: linear between the two keyframes around it, no shortest-arc logic; of keyframes that share a
    position the later one holds from there on.  A single keyframe is a constant."""
    out = []
    for p in positions:
        k = 0
        while k + 1 < len(path) and path[k + 1][0] <= p:
            k += 1
        if k + 1 == len(path):
            out.append(path[k][1])
            continue
        (p0, a0), (p1, a1) = path[k], path[k + 1]
        out.append(a0 + (a1 - a0) * ((p - p0) / (p1 - p0)))
    return out


def light_reduce(angle):
    """math.fmod(angle, 360), plus 360 when that is negative -> [0, 360).  (A negative angle so small that the sum rounds to 360, and -0.0, are 0.)"""
    r = math.fmod(angle, 360.0)
    if r < 0.0:
        r += 360.0
    return 0.0 if r >= 360.0 or r == 0.0 else r


def light_axis_side(reduced):
    """left | top | right | bottom when the reduced angle is exactly 0 / 90 / 180 / 270 (those frames take the existing ramp kernels), else None."""
    q = reduced / 90.0
    return LIGHT_AXIS_SIDES[int(q)] if q == int(q) and q * 90.0 == reduced else None


def light_dirs(angles):
    """(c, s) f64 per angle, the unit vector pointing AWAY from the light's side: exact multiples of 90 give exactly (1,0) (0,1) (-1,0) (0,-1),
    anything else (cos, sin) of math.radians of the reduced angle."""
    out = []
    for a in angles:
        r = light_reduce(a)
        side = light_axis_side(r)
        out.append(LIGHT_AXIS_DIRS[LIGHT_AXIS_SIDES.index(side)] if side is not None else (math.cos(math.radians(r)), math.sin(math.radians(r))))
    return out


def check_prompt_path(path, normal=False, highres_scale=1.0):
    """generation.prompt_path: None (off: nothing else is looked at) or keyframes [[pos, "prompt"], ...] -> [[float, str], ...]; anything else is a
    ValueError naming the key (run.py raises it before a model is loaded).  pos strictly increasing, the first 0 and (with more than one keyframe)
    the last 1 -- a single [[0, "p"]] is a constant path; every prompt a non-empty string.  Refused by both key names, as out of scope rather than
    impossible: generation.normal and a generation.highres_scale other than 1."""
    if path is None:
        return None
    if not isinstance(path, (list, tuple)) or len(path) == 0:
        raise ValueError(f"generation.prompt_path {path!r}: expected null or a list of keyframes [[pos, \"prompt\"], ...] with at least one")
    keys = []
    for kf in path:
        if (not isinstance(kf, (list, tuple)) or len(kf) != 2 or not _is_number(kf[0]) or not math.isfinite(kf[0])
                or not isinstance(kf[1], str) or not kf[1].strip()):
            raise ValueError(f"generation.prompt_path keyframe {kf!r}: expected [pos, \"prompt\"], a finite number and a non-empty string")
        keys.append([float(kf[0]), kf[1]])
    pos = [k[0] for k in keys]
    if pos[0] != 0.0 or (len(keys) > 1 and pos[-1] != 1.0) or any(b <= a for a, b in zip(pos, pos[1:])):
        raise ValueError(f"generation.prompt_path positions {pos}: expected strictly increasing values, the first 0 and (with more than one "
                         "keyframe) the last 1")
    if normal:
        raise ValueError("generation.prompt_path together with generation.normal is not supported: the four relights of the normal share one prompt")
    if isinstance(highres_scale, bool) or not isinstance(highres_scale, (int, float)) or float(highres_scale) != 1.0:
        raise ValueError(f"generation.prompt_path together with generation.highres_scale {highres_scale!r} is not supported: the second pass is "
                         "conditioned on one prompt")
    return keys


def prompt_sweep(prompt_a, prompt_b):
    """--prompt_sweep A B -> generation.prompt_path [[0, A], [1, B]]."""
    return [[0.0, str(prompt_a)], [1.0, str(prompt_b)]]


def prompt_table(path, n_total, lo=0, hi=None):
    """The per-frame text of generation.prompt_path for the run's frames lo <= i < hi (GLOBAL indices, positions as light_positions: a rank of a
    sharded run builds the rows of the frames it denoises).  -> (prompts, rows, index):
      prompts  the distinct keyframe prompts in order of first appearance (each is encoded once);
      rows     the distinct (k0, k1, t) of these frames in order of first appearance, k0 / k1 indices into `prompts` and t = (pos - p0)/(p1 - p0) in f64
               -- one embedding row each (tcl_text_lerp_f16);
      index    the row of every frame lo .. hi - 1.
    A frame that lands on a keyframe, and a segment whose two prompts are the same text, is (k, k, 0.0): the keyframe's own bits."""
    hi = n_total if hi is None else hi
    prompts, key = [], []
    for _, text in path:
        if text not in prompts:
            prompts.append(text)
        key.append(prompts.index(text))
    rows, index = [], []
    for p in light_positions(n_total, lo, hi):
        k = 0
        while k + 1 < len(path) and path[k + 1][0] <= p:
            k += 1
        if k + 1 == len(path) or path[k][0] == p or key[k] == key[k + 1]:
            row = (key[k], key[k], 0.0)
        else:
            p0, p1 = path[k][0], path[k + 1][0]
            row = (key[k], key[k + 1], (p - p0) / (p1 - p0))
        if row not in rows:
            rows.append(row)
        index.append(rows.index(row))
    return prompts, rows, index


IP_SCALE_DEFAULT = 0.6                 # generation.ip_adapter.scale when the block (or --ip_image alone) gives none
_IP_KEYS = ("image", "scale", "path")


def check_ip_adapter(block, normal=False, models=None, allow_random=False):
    """generation.ip_adapter: None (off: nothing else is looked at) or {image: <path>, scale: <float in [0, 2]>, path: <adapter file>} ->
    {image, scale, path, image_encoder} with the defaults filled in (scale IP_SCALE_DEFAULT, path models.ip_adapter).  run.py raises what is
    wrong before a model is loaded: a malformed block, a scale outside [0, 2] or an image that is no file is a ValueError naming the key; together with
    generation.normal a ValueError naming both keys (the four relights of a normal are lit by the ramps alone); a missing adapter file or
    models.image_encoder a FileNotFoundError, unless `allow_random` (models.allow_random / TCL_ALLOW_RANDOM_WEIGHTS=1) asks for seeded stand-ins."""
    import os
    if block is None:
        return None
    if not isinstance(block, dict) or not block or any(k not in _IP_KEYS for k in block):
        raise ValueError(f"generation.ip_adapter {block!r}: expected null or {{image: <path>, scale: <float in [0, 2]>, path: <adapter file>}}")
    image, scale, path = block.get("image"), block.get("scale", IP_SCALE_DEFAULT), block.get("path")
    if not isinstance(image, str) or not image:
        raise ValueError(f"generation.ip_adapter.image {image!r}: expected the path of the reference image")
    if not _is_number(scale) or not math.isfinite(scale) or not 0.0 <= float(scale) <= 2.0:
        raise ValueError(f"generation.ip_adapter.scale {scale!r}: expected a number in [0, 2]")
    if path is not None and (not isinstance(path, str) or not path):
        raise ValueError(f"generation.ip_adapter.path {path!r}: expected null (models.ip_adapter) or the path of the adapter file")
    if normal:
        raise ValueError("generation.ip_adapter together with generation.normal is not supported: the normal is computed from four relights that "
                         "differ in their ramp alone")
    if not os.path.isfile(image):
        raise ValueError(f"generation.ip_adapter.image {image!r}: no such file")
    models = models or {}
    path = path if path is not None else models.get("ip_adapter")
    encoder = models.get("image_encoder")
    if not allow_random:
        if not (path and os.path.isfile(path)):
            raise FileNotFoundError(f"IP-Adapter weights not found at {path!r} (generation.ip_adapter.path / models.ip_adapter: "
                                    "ip-adapter_sd15.safetensors or .bin); models.allow_random / TCL_ALLOW_RANDOM_WEIGHTS=1 stands seeded tensors in")
        if not (encoder and os.path.exists(encoder)):
            raise FileNotFoundError(f"CLIP ViT-H/14 image encoder not found at {encoder!r} (models.image_encoder: a snapshot with config.json and "
                                    "model.safetensors); models.allow_random / TCL_ALLOW_RANDOM_WEIGHTS=1 stands seeded tensors in")
    return dict(image=image, scale=float(scale), path=path, image_encoder=encoder)


DETAIL_MODES = ("add", "ratio")          # generation.detail_transfer.mode, in the order of TCL_DETAIL_ADD / TCL_DETAIL_RATIO
DETAIL_CHANNELS = ("rgb", "luma")        # generation.detail_transfer.channels
DETAIL_SIGMA = (0.5, 16.0)               # the radius ceil(3 sigma) stays within the kernel's 48
DETAIL_DEFAULTS = dict(sigma=3.0, mode="add", blend=1.0, channels="rgb")


def check_detail(block, normal=False, iclight_model="fc", fbc_matting=True):
    """generation.detail_transfer: None (off: nothing else is looked at) or {sigma, mode: add | ratio, blend, channels: rgb | luma} -> the block with
    the defaults filled in (DETAIL_DEFAULTS); a bare number is {sigma: number}.  run.py and Generator raise what is wrong before a model is loaded,
    each by the name of its key: an unknown key, a sigma outside DETAIL_SIGMA, a blend outside [0, 1], an unknown mode or channels.  Refused by both
    key names: generation.normal (its outputs are ratios of four relights, not a relight), and iclight_model fbc with fbc_matting false (an fbc run
    may carry a new background; without the matte as the weight the old background would ghost into it)."""
    if block is None:
        return None
    if _is_number(block):
        block = dict(sigma=block)
    if not isinstance(block, dict) or any(k not in DETAIL_DEFAULTS for k in block):
        raise ValueError(f"generation.detail_transfer {block!r}: expected null, a number (sigma) or {{sigma: <float>, mode: add | ratio, "
                         "blend: <float in [0, 1]>, channels: rgb | luma}")
    out = dict(DETAIL_DEFAULTS, **block)
    sigma, blend = out["sigma"], out["blend"]
    if not _is_number(sigma) or not DETAIL_SIGMA[0] <= float(sigma) <= DETAIL_SIGMA[1]:
        raise ValueError(f"generation.detail_transfer.sigma {sigma!r}: expected a number in [{DETAIL_SIGMA[0]}, {DETAIL_SIGMA[1]}]")
    if not _is_number(blend) or not 0.0 <= float(blend) <= 1.0:
        raise ValueError(f"generation.detail_transfer.blend {blend!r}: expected a number in [0, 1]")
    for key, allowed in (("mode", DETAIL_MODES), ("channels", DETAIL_CHANNELS)):
        if not isinstance(out[key], str) or out[key].lower() not in allowed:
            raise ValueError(f"generation.detail_transfer.{key} {out[key]!r}: expected one of {' | '.join(allowed)}")
        out[key] = out[key].lower()
    out["sigma"], out["blend"] = float(sigma), float(blend)
    if normal:
        raise ValueError("generation.detail_transfer together with generation.normal is not supported: the normal's outputs are ratios of four "
                         "relights, not a relight")
    model = "fc" if iclight_model is None else str(iclight_model).lower()
    if model == "fbc" and not fbc_matting:
        raise ValueError("generation.detail_transfer under generation.iclight_model fbc needs generation.fbc_matting: true: the matte is the step's "
                         "weight, without it the source's background would ghost into a new one")
    return out


KEYFRAME_MAX_INTERVAL = 16               # TCL_KEYFRAME_MAX_GAP: the longest chain of flows tcl_flow_chain_f32 composes
# alpha, diff_threshold: the reference's own (compute_fwdbwd_mask(alpha=0.1), get_mask_bwds(diff_threshold=0.1), utils/flow_utils.py); eps = 1/64 is a
# definition: the floor under numerator and denominator of the gain, a power of two so that adding and removing it is exact on lattice inputs
KEYFRAME_DEFAULTS = dict(interval=4, alpha=0.1, diff_threshold=0.1, eps=0.015625)


def check_keyframes(block, normal=False, light_path=None, prompt_path=None, scene_type="video", post_opt_mode="replicated", shard_post_opt=False):
    """generation.keyframes: None (off: nothing else is looked at), a bare integer K or {interval: K, alpha, diff_threshold, eps} -> the block with
    the defaults filled in (KEYFRAME_DEFAULTS), or None for interval 1 -- the key switched off: every frame is a key, nothing is launched and nothing
    is recorded, like blend 0 of detail transfer.  Each fault is a ValueError naming its key: an unknown key, an interval that is no integer in
    [1, KEYFRAME_MAX_INTERVAL], alpha or diff_threshold not > 0, eps outside (0, 0.25].  With interval > 1, refused by both key names as out of scope
    (not impossible): generation.normal (its outputs are ratios of four relights), generation.light_path and generation.prompt_path (their
    per-frame positions belong to the full clip), data.scene_type sceneflow (its producer hands on past flows only), post_opt_mode shard /
    shard_post_opt (propagation needs the keys on both sides of a rank's block)."""
    if block is None:
        return None
    if isinstance(block, int) and not isinstance(block, bool):
        block = dict(interval=block)
    if not isinstance(block, dict) or "interval" not in block or any(k not in KEYFRAME_DEFAULTS for k in block):
        raise ValueError(f"generation.keyframes {block!r}: expected null, an integer (interval) or {{interval: <int in [1, {KEYFRAME_MAX_INTERVAL}]>, "
                         "alpha: <float > 0>, diff_threshold: <float > 0>, eps: <float in (0, 0.25]>}")
    out = dict(KEYFRAME_DEFAULTS, **block)
    k = out["interval"]
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KEYFRAME_MAX_INTERVAL:
        raise ValueError(f"generation.keyframes.interval {k!r}: expected an integer in [1, {KEYFRAME_MAX_INTERVAL}]")
    for key in ("alpha", "diff_threshold"):
        if not _is_number(out[key]) or not 0.0 < float(out[key]) < float("inf"):
            raise ValueError(f"generation.keyframes.{key} {out[key]!r}: expected a number > 0")
        out[key] = float(out[key])
    if not _is_number(out["eps"]) or not 0.0 < float(out["eps"]) <= 0.25:
        raise ValueError(f"generation.keyframes.eps {out['eps']!r}: expected a number in (0, 0.25]")
    out["eps"] = float(out["eps"])
    if k == 1:
        return None
    if normal:
        raise ValueError("generation.keyframes together with generation.normal is not supported: the normal's outputs are ratios of four relights, "
                         "not a relight")
    for key, v in (("light_path", light_path), ("prompt_path", prompt_path)):
        if v is not None:
            raise ValueError(f"generation.keyframes together with generation.{key} is not supported: the path's per-frame positions belong to the "
                             "full clip, not to the keyframes")
    if str(scene_type).lower() == "sceneflow":
        raise ValueError("generation.keyframes together with data.scene_type sceneflow is not supported: its producer hands on past flows only, "
                         "propagation needs both directions")
    if shard_post_opt or str(post_opt_mode) == "shard":
        raise ValueError("generation.keyframes together with post_opt_mode shard (shard_post_opt) is not supported: propagation needs the keys on "
                         "both sides of a rank's block")
    return out


def keyframe_ids(n, interval):
    """The key frames of an n-frame run: 0, K, 2K, ... plus n - 1 when it is not one of them, so every other frame has a key on each side."""
    n, interval = int(n), int(interval)
    if n < 1 or interval < 1:
        raise ValueError(f"keyframe_ids: n {n} and interval {interval} must be at least 1")
    ids = list(range(0, n, interval))
    if ids[-1] != n - 1:
        ids.append(n - 1)
    return ids


NOISE_WARP_DEFAULTS = dict(steps=True)    # generation.noise_warp: is the per-step noise of the SDE solver a warped chain too?


def check_noise_warp(noise_mode, block=None, keyframes=None, highres_scale=1.0, normal=False):
    """generation.noise_mode warp and its block generation.noise_warp: {steps: <bool>} -> the block with the defaults filled in (NOISE_WARP_DEFAULTS),
    or None under every other noise_mode -- the block is read under warp only, and what an unknown mode raises stays with Generator._draw_start.
    Each fault is a ValueError naming its key: a block that is no mapping, an unknown key, a steps that is no bool.  Refused by both key names as out
    of scope: generation.keyframes (the flows of consecutive frames do not connect key frames), generation.highres_scale > 1 (the flows live at the
    final size, the first denoise at the working size), generation.normal."""
    if not isinstance(noise_mode, str) or noise_mode.lower() != "warp":
        return None
    if block is not None and (not isinstance(block, dict) or any(k not in NOISE_WARP_DEFAULTS for k in block)):
        raise ValueError(f"generation.noise_warp {block!r}: expected null or {{steps: <bool>}}")
    out = dict(NOISE_WARP_DEFAULTS, **(block or {}))
    if not isinstance(out["steps"], bool):
        raise ValueError(f"generation.noise_warp.steps {out['steps']!r}: expected true or false")
    if keyframes is not None:
        raise ValueError("generation.noise_mode warp together with generation.keyframes is not supported: the flows of consecutive frames do not "
                         "connect key frames")
    if highres_scale is not None and float(highres_scale) > 1.0:
        raise ValueError("generation.noise_mode warp together with generation.highres_scale > 1 is not supported: the flows live at the final size, "
                         "the first denoise at the working size")
    if normal:
        raise ValueError("generation.noise_mode warp together with generation.normal is not supported: the four relights start from one noise and "
                         "no flows are estimated")
    return out


FULLRES_GUIDES = ("rgb", "luma")         # generation.fullres.guide, in the order of the kernel's `luma` argument (0 / 1)
FULLRES_RADIUS = (1, 64)                 # TCL_GUIDED_MAX_RADIUS
FULLRES_EPS = (1e-4, 1.0)                # the floor of the fit's denominator: the kernel's error bound scales like 1 / eps
FULLRES_DEFAULTS = dict(radius=8, eps=1e-3, guide="rgb")


def check_fullres(block, normal=False, iclight_model="fc", background_cond=False, scene_type="video"):
    """generation.fullres: None or false (off: nothing else is looked at), true (the defaults), a bare integer radius or {radius, eps, guide: rgb |
    luma} -> the block with the defaults filled in (FULLRES_DEFAULTS).  Each fault is a ValueError naming its key: an unknown key, a radius that is
    no integer in FULLRES_RADIUS, an eps outside FULLRES_EPS, an unknown guide.  Refused by both key names: generation.normal (its outputs are
    ratios of four relights), generation.iclight_model fbc and background_cond (the new background is not in the source's pixels, so no gain on them
    reproduces it), and data.scene_type sceneflow (its parser reads the frames its own way: out of scope, not impossible)."""
    if block is None or block is False:
        return None
    if block is True:
        block = {}
    elif isinstance(block, int):
        block = dict(radius=block)
    if not isinstance(block, dict) or any(k not in FULLRES_DEFAULTS for k in block):
        raise ValueError(f"generation.fullres {block!r}: expected null, true, an integer (radius) or {{radius: <int in [{FULLRES_RADIUS[0]}, "
                         f"{FULLRES_RADIUS[1]}]>, eps: <float in [{FULLRES_EPS[0]}, {FULLRES_EPS[1]}]>, guide: rgb | luma}}")
    out = dict(FULLRES_DEFAULTS, **block)
    radius, eps, guide = out["radius"], out["eps"], out["guide"]
    if isinstance(radius, bool) or not isinstance(radius, int) or not FULLRES_RADIUS[0] <= radius <= FULLRES_RADIUS[1]:
        raise ValueError(f"generation.fullres.radius {radius!r}: expected an integer in [{FULLRES_RADIUS[0]}, {FULLRES_RADIUS[1]}]")
    if not _is_number(eps) or not FULLRES_EPS[0] <= float(eps) <= FULLRES_EPS[1]:
        raise ValueError(f"generation.fullres.eps {eps!r}: expected a number in [{FULLRES_EPS[0]}, {FULLRES_EPS[1]}]")
    if not isinstance(guide, str) or guide.lower() not in FULLRES_GUIDES:
        raise ValueError(f"generation.fullres.guide {guide!r}: expected one of {' | '.join(FULLRES_GUIDES)}")
    out["eps"], out["guide"] = float(eps), guide.lower()
    if normal:
        raise ValueError("generation.fullres together with generation.normal is not supported: the normal's outputs are ratios of four relights, "
                         "not a relight")
    if (iclight_model is not None and str(iclight_model).lower() == "fbc") or background_cond:
        key = "generation.background_cond" if background_cond else "generation.iclight_model fbc"
        raise ValueError(f"generation.fullres together with {key} is not supported: the new background is not in the source's pixels, so no "
                         "gain and offset on them gives it back")
    if str(scene_type).lower() == "sceneflow":
        raise ValueError("generation.fullres together with data.scene_type sceneflow is not supported: its parser reads the frames its own way "
                         "(out of scope, not impossible)")
    return out


# what resolve_generation normalises: run.py writes these back into the configuration (config.yaml records them), Generator into its cfg
RESOLVED_KEYS = ("init_latent", "init_strength", "highres_scale", "highres_denoise", "iclight_model", "bg_source", "light_path", "prompt_path")


def resolve_generation(cfg):
    """The one resolution of the generation options, for run.py (before a model is loaded) and Generator alike.  cfg: generate.DEFAULTS overlaid
    with generation.*, post_opt.* and background_cond.  Every check_* above runs once, in this order, so two faults at once are reported the same
    way everywhere; check_ip_adapter (models, the file system) is the caller's.  -> the RESOLVED_KEYS normalised, and what follows from them:
    fbc / light / img2img / highres, normal_sides (() unless generation.normal), schedule = (scheduler steps, begin index, steps executed) -- the
    whole n_timesteps unless the start is an img2img one -- and schedule_highres (the second pass's; None when it is off).  generation.keyframes
    (check_keyframes; cfg may carry data.scene_type as scene_type) is checked here too; its normalised block is in the result as "keyframes" only
    when the key is on (interval > 1), so a run without it resolves to exactly what it did; likewise "noise_warp" (check_noise_warp), in the result
    under noise_mode warp only, and "fullres" (check_fullres; cfg may carry data.scene_type as scene_type), in the result only when the key is on."""
    n, normal, bg_cond = cfg["n_timesteps"], cfg["normal"], bool(cfg.get("background_cond"))
    r = {}
    r["init_latent"], r["init_strength"] = check_init(cfg["init_latent"], cfg["init_strength"], n)
    r["highres_scale"], r["highres_denoise"] = check_highres(cfg["highres_scale"], cfg["highres_denoise"], n, bg_cond)
    r["iclight_model"], r["bg_source"] = check_fbc(cfg["iclight_model"], cfg["bg_source"], r["init_latent"], r["highres_scale"], bg_cond)
    r["light_path"] = check_light_path(cfg["light_path"], r["init_latent"], normal, r["iclight_model"], r["bg_source"], r["init_strength"], n)
    r["normal_sides"] = check_normal(normal, r["iclight_model"], cfg["fbc_matting"], cfg["apply_opt"])
    r["prompt_path"] = check_prompt_path(cfg["prompt_path"], normal, r["highres_scale"])
    keyframes = check_keyframes(cfg.get("keyframes"), bool(normal), r["light_path"], r["prompt_path"], cfg.get("scene_type", "video"),
                                cfg.get("post_opt_mode", "replicated"), bool(cfg.get("shard_post_opt")))
    if keyframes is not None:
        r["keyframes"] = keyframes
    noise_warp = check_noise_warp(cfg.get("noise_mode"), cfg.get("noise_warp"), keyframes, r["highres_scale"], bool(normal))
    if noise_warp is not None:
        r["noise_warp"] = noise_warp
    fullres = check_fullres(cfg.get("fullres"), bool(normal), r["iclight_model"], bg_cond, cfg.get("scene_type", "video"))
    if fullres is not None:
        r["fullres"] = fullres
    r["fbc"], r["light"], r["highres"] = r["iclight_model"] == "fbc", r["light_path"] is not None, r["highres_scale"] != 1.0
    r["img2img"] = r["init_latent"] != "none" or (r["light"] and not r["fbc"])      # fc: the path's ramps are the start
    r["schedule"] = img2img_schedule(n, r["init_strength"]) if r["img2img"] else (n, 0, n)
    r["schedule_highres"] = img2img_schedule(n, r["highres_denoise"]) if r["highres"] else None
    return r


TOME_MAX_SRC_TOKENS = 64 * 1024      # tcl_tome_match_f16 / _affine_f16: source tokens of one match (csrc/merge.hip)


def check_highres_tokens(H2, W2, chunk_size):
    """The second pass runs VidToMe on chunks of `chunk_size` frames at (H2, W2): one frame is the destination, the others' level-0 tokens are the
    sources of one match, and the match kernels take at most TOME_MAX_SRC_TOKENS of them.  1920x1088 with chunk_size 4 (97 920) is refused here,
    before a model is loaded, instead of inside the loop; chunk_size 2 (32 640) or a smaller scale fits."""
    n = (int(chunk_size) - 1) * (int(H2) // 8) * (int(W2) // 8)
    if n > TOME_MAX_SRC_TOKENS:
        raise ValueError(f"generation.highres_scale: the final size {H2}x{W2} with generation.chunk_size {chunk_size} gives {n} source tokens per VidToMe "
                         f"match, more than the {TOME_MAX_SRC_TOKENS} the match kernels take -- lower highres_scale or chunk_size")


def shard_range(n, rank, world):
    """Contiguous frame block of `rank` (sizes differ by at most one; SURVEY 8(d) config 3: 38/38/38/38/37/37/37/37)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def expon_lr(step, lr_init, lr_final, max_steps):
    """get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, max_steps=max_steps)(step)  (utils/general_utils.py:31-64, delay off)."""
    t = min(max(step / max_steps, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def pad8_amounts(H, W):
    """eval_utils.InputPadder -> (left, right, top, bottom) up to multiples of 8, split as evenly as possible."""
    ph, pw = (((H // 8) + 1) * 8 - H) % 8, (((W // 8) + 1) * 8 - W) % 8
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def memflow_splitkv_chunks(P, T, want=3):
    """Key chunks of MemFlowNet's memory-read attention (P queries, T keys, one head): tcl_attention_splitkv_f16 takes chunks of a multiple of 64
    keys and at most 1024 blocks of 128 queries x chunks.  `want` if it fits, else the first of (3, 2, 5, 4, 6) that does, else 0 = the one-pass
    kernel; a `want` below 2 asks for the one-pass kernel."""
    fits = lambda c: T % (64 * c) == 0 and -(-P // 128) * c <= 1024
    if want < 2:
        return 0
    return want if fits(want) else next((c for c in (3, 2, 5, 4, 6) if fits(c)), 0)
