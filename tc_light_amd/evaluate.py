"""warp-error-ssim, the temporal-consistency figure of the reference's evaluate.py (evaluate.py:1-133, utils/evaluation/eval_utils.py:252-350).

For every pair of neighbouring frames (i, i+1) of a relit video, RAFT estimates the forward and backward flow between the SOURCE frames i and i+1
(20 iterations, test mode, the frames in 0..255 and replicate-padded to multiples of 8, the flows unpadded); the relit frame i is warped onto
frame i+1 along the backward flow with a cubic remap, pixels failing the forward-backward consistency check are zeroed in both frames, and the
score of the pair is the SSIM of the two uint8 images.  The metric is the mean over the pairs.  RAFT is `raft.RAFTEngine` through
`raft.estimate_flows_raft` (fwd = fut[i], bwd = past[i+1]); the warp, mask and SSIM are the kernels of csrc/evaluate.hip.

clip-frame and clip-text (evaluate.py:39-49, eval_utils.py:129-161) are computed when a CLIP checkpoint is configured (`models.clip` / --clip): the
frames go through `clip.CLIPEngine.encode_image`, clip-frame is the mean off-diagonal cosine between the frame features and clip-text the mean cosine
of the frame features to the prompt's text feature (tcl_clip_scores).  With no CLIP path nothing of it is loaded and the two figures are listed as not
computed, as before.

pick-score (evaluate.py:52-56, eval_utils.py:163-176) is computed when a PickScore_v1 checkpoint is configured (`models.pick` / --pick): the same
engine at CLIP ViT-H/14 (`clip.pick_engine`: 16 heads per tower, erf GELU, patch rows padded from 588 to 640 columns, the transformers processor's
floored centre crop), the prompt tokenised as the processor does (truncated to 77, unpadded), and exp(logit_scale) cos(text, frame) averaged over the
frames (tcl_pick_scores).

frame-lpips (eval_utils.py:368-386 FrameLPIPS, which the reference ships but its evaluate.py never calls) is computed when a VGG-16 state dict is
configured (`models.lpips_vgg` / --lpips, with `models.lpips_lin` / --lpips_lin for LPIPS's linear layers): the LPIPS-VGG distance (`lpips.LPIPSEngine`)
between every relit frame but the last and its source frame, both in 0..255 and replicate-padded to multiples of 8, averaged over the frames.  It asks
whether the relit video is still the same video, which none of the other figures does.  With no path it is not loaded and result.txt is what it was.
"""
import math
import os

import numpy as np
import torch

from . import clip
from .flow_core import pad8
from .lib import lib, stream
from .raft import estimate_flows_raft

EDIT_STEMS = ("output_opt", "output")          # evaluate.py:27: output_opt.mp4 if it exists, else output.mp4
SOURCE_STEM = "output_gt"                       # evaluate.py:28
VIDEO_EXTS = (".mp4", ".avi")                   # .avi: what dataparser.save_video writes without an H.264 encoder
NOT_COMPUTED = ("clip-frame", "clip-text", "pick-score")


def not_computed(clip_on, pick_on=False):
    """The figures of the reference's table this run leaves out: the two clip-* figures without a CLIP checkpoint, pick-score without a PickScore one."""
    return tuple(m for m in NOT_COMPUTED if not (clip_on and m.startswith("clip-")) and not (pick_on and m == "pick-score"))


def clip_settings(models, clip_arg=None, tokenizer_arg=None):
    """-> (CLIP checkpoint path or None, tokenizer directory or None).  The path is --clip, else `models.clip`; None switches the CLIP figures off
    (allow_random alone never switches them on).  The tokenizer directory is --clip_tokenizer, else `models.clip_tokenizer`, else
    `models.text_encoder`."""
    models = models or {}
    path = clip_arg or models.get("clip") or None
    tok = tokenizer_arg or models.get("clip_tokenizer") or models.get("text_encoder") or None
    return path, (tok if path else None)


def pick_settings(models, pick_arg=None, tokenizer_arg=None):
    """-> (PickScore checkpoint path or None, tokenizer directory or None).  The path is --pick, else `models.pick`; None switches pick-score off
    (allow_random alone never switches it on).  The tokenizer directory is --pick_tokenizer, else `models.pick_tokenizer`, else the checkpoint
    directory itself when it holds a vocab.json, else `models.clip_tokenizer`, else `models.text_encoder` (one BPE vocabulary serves them all)."""
    models = models or {}
    path = pick_arg or models.get("pick") or None
    own = path if path and os.path.isfile(os.path.join(path, "vocab.json")) else None
    tok = tokenizer_arg or models.get("pick_tokenizer") or own or models.get("clip_tokenizer") or models.get("text_encoder") or None
    return path, (tok if path else None)


def lpips_settings(models, lpips_arg=None, lin_arg=None):
    """-> (VGG-16 state dict path or None, LPIPS linear-layer path or None).  The first is --lpips, else `models.lpips_vgg`; None switches
    frame-lpips off (allow_random alone never switches it on).  The second is --lpips_lin, else `models.lpips_lin`, and counts only when the
    figure is on."""
    models = models or {}
    path = lpips_arg or models.get("lpips_vgg") or None
    lin = lin_arg or models.get("lpips_lin") or None
    return path, (lin if path else None)


# ---- the kernels
def warp_mask_planes(edit_u8, fut, past, i0, B):
    """Pairs i0 .. i0+B-1 -> (warped, target) uint8 [B,H,W,3] on the device.  edit_u8 [N,H,W,3] uint8, fut / past [N,2,H,W] f32 (device)."""
    N, H, W = edit_u8.shape[:3]
    dev = fut.device
    warped = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    target = torch.empty_like(warped)
    lib().tcl_eval_warp_mask_u8(edit_u8, fut, past, warped, target, N, H, W, i0, B, stream())
    return warped, target


def ssim_u8(x, y):
    """x, y uint8 [B,H,W,3] on the device -> f64 [B]: skimage structural_similarity(channel_axis=2) with its defaults, per plane pair."""
    B, H, W = x.shape[:3]
    if x.shape != y.shape or x.shape[-1] != 3 or x.dtype != torch.uint8 or y.dtype != torch.uint8:
        raise ValueError(f"ssim_u8 takes two uint8 [B,H,W,3] tensors of one shape, got {tuple(x.shape)} {x.dtype} / {tuple(y.shape)} {y.dtype}")
    if H < 7 or W < 7:
        raise ValueError(f"SSIM's 7x7 window needs H, W >= 7, got {H}x{W}")
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    L = lib()
    ws = torch.empty(L.tcl_eval_ssim_workspace_bytes(B, H, W), dtype=torch.uint8, device=x.device)
    L.tcl_eval_ssim_u8(x.contiguous(), y.contiguous(), out, B, H, W, ws, stream())
    return out


def warp_ssim_from_flows(edit_u8, fut, past, batch=4):
    """edit_u8 [N,H,W,3] uint8 (the relit frames), fut / past [N,2,H,W] f32 (estimate_flows_raft's layout, on the device) ->
    (mean over the N-1 pairs, per-pair float64 numpy array).  Pairs run `batch` at a time."""
    N, H, W = edit_u8.shape[:3]
    if N < 2:
        raise ValueError(f"warp-error-ssim needs at least 2 frames, got {N}")
    if tuple(fut.shape) != (N, 2, H, W) or tuple(past.shape) != (N, 2, H, W):
        raise ValueError(f"flows must be [N,2,H,W] = {(N, 2, H, W)}, got {tuple(fut.shape)} / {tuple(past.shape)}")
    if H < 7 or W < 7:
        raise ValueError(f"SSIM's 7x7 window needs H, W >= 7, got {H}x{W}")
    dev = fut.device
    e = torch.as_tensor(edit_u8).to(dev).contiguous()
    if e.dtype != torch.uint8 or e.shape[-1] != 3:
        raise ValueError(f"edit frames must be uint8 [N,H,W,3], got {e.dtype} {tuple(e.shape)}")
    fut, past = fut.float().contiguous(), past.float().contiguous()
    L = lib()
    batch = max(1, min(batch, N - 1))
    scores = torch.empty(N - 1, dtype=torch.float64, device=dev)
    warped = torch.empty(batch, H, W, 3, dtype=torch.uint8, device=dev)
    target = torch.empty_like(warped)
    ws = torch.empty(L.tcl_eval_ssim_workspace_bytes(batch, H, W), dtype=torch.uint8, device=dev)
    for s in range(0, N - 1, batch):
        b = min(batch, N - 1 - s)
        L.tcl_eval_warp_mask_u8(e, fut, past, warped, target, N, H, W, s, b, stream())
        L.tcl_eval_ssim_u8(warped, target, scores[s:], b, H, W, ws, stream())
    per = scores.cpu().numpy()
    return float(np.mean(per)), per


def resize_like(source_u8, H, W):
    """PIL Image.resize((W, H)) with its default filter on every frame (evaluate.py:34-35), uint8 [N,h,w,3] -> [N,H,W,3]."""
    from PIL import Image
    src = source_u8.cpu().numpy()
    return torch.from_numpy(np.stack([np.asarray(Image.fromarray(f).resize((W, H))) for f in src]))


@torch.no_grad()
def warp_ssim(edit_u8, source_u8, raft_engine, batch=4):
    """The reference's SaveWarpingImage with RAFT flows (flow lists None): edit_u8 / source_u8 uint8 [N,H,W,3] (numpy or tensors) ->
    (warp-error-ssim, per-pair float64 array).  Source frames of another size are resized to the edit size first (PIL, default filter)."""
    from .raft import check_size
    edit, src = clip.nhwc_u8(edit_u8), clip.nhwc_u8(source_u8)
    N, H, W = edit.shape[:3]
    if N < 2 or len(src) < N:
        raise ValueError(f"warp-error-ssim needs at least 2 edit frames and as many source frames, got {N} / {len(src)}")
    if tuple(src.shape[1:3]) != (H, W):
        src = resize_like(src, H, W)
    x = src[:N].to(raft_engine.dev).permute(0, 3, 1, 2).float()            # load_image: float 0..255
    x, pad = pad8(x)
    check_size(*x.shape[-2:])
    fut, past = estimate_flows_raft(raft_engine, x, batch=batch)            # 0..255 in: RAFT's own normalisation is then the right one
    del x
    l, r, t, b = pad
    Hp, Wp = fut.shape[-2:]
    if any(pad):
        fut = fut[..., t:Hp - b, l:Wp - r].contiguous()
        past = past[..., t:Hp - b, l:Wp - r].contiguous()
    return warp_ssim_from_flows(edit, fut, past, batch=batch)


# ---- the CLIP figures
def _features(edit_u8, engine, batch, features):
    """The image features of the frames (encode_image checks them: uint8 [N,H,W,3]), unless the caller has them already."""
    return engine.encode_image(edit_u8, batch=batch) if features is None else features


@torch.no_grad()
def clip_frame(edit_u8, engine, batch=64, features=None):
    """eu.clip_frame (eval_utils.py:146-161): the sum of the off-diagonal cosines between the frame features / (N (N - 1)).  edit_u8 uint8 [N,H,W,3]."""
    feats = _features(edit_u8, engine, batch, features)
    if feats.shape[0] < 2:
        raise ValueError(f"clip-frame needs at least 2 frames, got {feats.shape[0]}")
    return clip.scores(feats)[0]


def prompt_id_rows(prompt, tokenizer, context=77, allow_random=False):
    """The token rows clip-text is computed from: the whole prompt when it fits the context, else (evaluate.py:43-49) its non-empty parts between
    full stops, whose scores are averaged."""
    try:
        return [clip.tokenize(prompt, tokenizer, context, allow_random)]
    except RuntimeError:
        print(f"[WARN] Prompt too long: '{prompt}', splitting.")
        return [clip.tokenize(p, tokenizer, context, allow_random) for p in prompt.split(".") if p.strip()]


def _text_score(feats, ids, engine):
    return clip.scores(feats, engine.encode_text(ids)[0])[1]


@torch.no_grad()
def clip_text(edit_u8, prompt, engine, tokenizer, allow_random=False, batch=64, features=None):
    """eu.clip_text (eval_utils.py:129-144) with evaluate.py:41-49's fallback: the mean cosine of the frame features to the prompt's text feature."""
    feats = _features(edit_u8, engine, batch, features)
    rows = prompt_id_rows(prompt, tokenizer, engine.context, allow_random)
    if not rows:
        raise ValueError(f"empty prompt {prompt!r}: nothing to score")
    return float(np.mean([_text_score(feats, ids, engine) for ids in rows]))


# ---- pick-score
@torch.no_grad()
def pick_score(edit_u8, prompt, engine, tokenizer, allow_random=False, batch=64, features=None):
    """eu.pick_score_func (eval_utils.py:163-176) averaged over the frames (evaluate.py:52-56): exp(logit_scale) times the cosine of the prompt's
    text embedding to every frame's image embedding.  `engine` is clip.pick_engine's; `features` are its image features when already computed."""
    if engine.logit_scale is None:
        raise ValueError("pick-score needs the checkpoint's logit_scale, which this state dict lacks")
    feats = _features(edit_u8, engine, batch, features)
    ids = clip.tokenize_truncated(prompt, tokenizer, engine.context, allow_random)
    return clip.pick_scores(feats, engine.encode_text(ids)[0], engine.logit_scale)[0]


# ---- frame-lpips
@torch.no_grad()
def frame_lpips(edit_u8, source_u8, engine, batch=4):
    """eu.FrameLPIPS (eval_utils.py:368-386): edit_u8 / source_u8 uint8 [N,H,W,3] (numpy or tensors) -> (the mean LPIPS-VGG distance between relit
    frame i and source frame i over i = 0 .. N-2, the per-frame float64 array).  The reference's own behaviour is kept: the last frame is left out
    (`edit_pil_list[:-1]`), the frames stay in 0..255 (load_image; LPIPS's normalize=False) and both are replicate-padded to multiples of 8
    (InputPadder) before the distance.  Source frames of another size are resized to the edit size first, as for the other figures.  `engine` is a
    lpips.LPIPSEngine; `batch` pairs run at a time."""
    from .lpips import pad8_u8
    edit, src = clip.nhwc_u8(edit_u8), clip.nhwc_u8(source_u8)
    N, H, W = edit.shape[:3]
    if N < 2 or len(src) < N - 1:
        raise ValueError(f"frame-lpips leaves the last frame out: it needs at least 2 edit frames and one source frame fewer, got {N} / {len(src)}")
    src = src[:N - 1]
    if tuple(src.shape[1:3]) != (H, W):
        src = resize_like(src, H, W)
    batch = max(1, min(batch, N - 1))
    per = []
    for s in range(0, N - 1, batch):
        e = pad8_u8(edit[s:min(s + batch, N - 1)].to(engine.dev))
        g = pad8_u8(src[s:s + batch].to(engine.dev))
        per.append(engine.distance(g, e))                                   # loss_fn_vgg(gt, pil_img)
    per = torch.cat(per).cpu().numpy().astype(np.float64)
    return float(np.mean(per)), per


# ---- light-follow
def light_follow(edit_u8, source_u8, wanted, device="cuda"):
    """edit_u8 / source_u8 uint8 [N,H,W,3] (numpy or tensors), wanted: the N wanted angles in degrees (lightfit.wanted_angles) ->
    (light-follow, light-contrast, per-frame list of dicts; lightfit.figures).  Source frames of another size are resized to the edit size first, as
    for the other figures; the sums run on `device` (tcl_light_fit_u8), the 3x3 solves on the host in f64."""
    from . import lightfit
    edit, src = clip.nhwc_u8(edit_u8), clip.nhwc_u8(source_u8)
    N, H, W = edit.shape[:3]
    if N < 1 or len(src) < N:
        raise ValueError(f"light-follow needs at least 1 edit frame and as many source frames, got {N} / {len(src)}")
    if len(wanted) != N:
        raise ValueError(f"light-follow: {len(wanted)} wanted angles for {N} frames")
    src = src[:N]
    if tuple(src.shape[1:3]) != (H, W):
        src = resize_like(src, H, W)
    e = edit.to(device).permute(0, 3, 1, 2).contiguous()
    s = src.to(device).permute(0, 3, 1, 2).contiguous()
    return lightfit.figures(lightfit.light_sums(e, s).cpu().numpy(), wanted)


# ---- files
def find_videos(output_dir):
    """-> (edit path, source path) in the reference's order: output_opt, then output, each as .mp4 then .avi, then output.npy for the edit;
    output_gt as .mp4, then .avi, then .npy for the source.  FileNotFoundError when either is missing."""
    def first(stems, tail):
        for s in stems:
            for ext in VIDEO_EXTS:
                p = os.path.join(output_dir, s + ext)
                if os.path.exists(p):
                    return p
        p = os.path.join(output_dir, tail)
        return p if os.path.exists(p) else None
    edit = first(EDIT_STEMS, "output.npy")
    source = first((SOURCE_STEM,), SOURCE_STEM + ".npy")
    if edit is None:
        raise FileNotFoundError(f"no relit video in {output_dir} (output_opt / output as .mp4 or .avi, or output.npy)")
    if source is None:
        raise FileNotFoundError(f"no source video in {output_dir} ({SOURCE_STEM}.mp4 / .avi / .npy)")
    return edit, source


def read_video_u8(path):
    """A video file -> uint8 [N,H,W,3] with the decoded values exactly (no float round trip)."""
    from .dataparser import read_mjpeg_avi
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim == 4 and a.shape[1] == 3 and a.shape[-1] != 3:
            a = a.transpose(0, 2, 3, 1)
        if a.dtype != np.uint8:
            raise ValueError(f"{path}: expected uint8 frames, got {a.dtype}")
        return torch.from_numpy(np.ascontiguousarray(a))
    if path.lower().endswith(".avi"):
        fr = read_mjpeg_avi(path)
        if fr is not None:
            return fr
    try:
        import torchvision.io as tvio
        return tvio.read_video(path, pts_unit="sec", output_format="THWC")[0]
    except ImportError:
        pass
    try:
        import cv2
    except ImportError:
        raise RuntimeError(f"no video decoder (torchvision.io / cv2) for {path}; write the frames as a Motion-JPEG .avi or a uint8 .npy") from None
    cap, out = cv2.VideoCapture(path), []
    while True:
        ok, fr = cap.read()
        if not ok:
            break
        out.append(torch.from_numpy(fr[..., ::-1].copy()))
    if not out:
        raise RuntimeError(f"cv2 decoded no frames from {path}")
    return torch.stack(out)


# ---- the report
def video_name(config):
    """evaluate.py:123: the parent directory of config.input_path, else 'unknown_video'."""
    p = config.get("input_path") if hasattr(config, "get") else None
    return p.split("/")[-2] if isinstance(p, str) and "/" in p else "unknown_video"


def cost_scores(config, width, height):
    """evaluate.py:61-66 (--eval_cost): the z_* entries from the run's config.yaml."""
    missing = [k for k in ("sec_per_frame", "max_memory_allocated", "total_number_of_frames", "total_time") if k not in config]
    if missing:
        raise KeyError(f"--eval_cost needs {missing} in config.yaml (written by run.py)")
    return {"z_fps": 1 / config["sec_per_frame"], "z_max_memory_allocated(M)": config["max_memory_allocated"],
            "z_resolution": math.sqrt(width * height), "z_total_frames": config["total_number_of_frames"], "z_total_time(s)": config["total_time"]}


def format_results(name, prompt, scores):
    """print_and_save_results (evaluate.py:70-95): the header `{name} - {prompt}`, then the metrics sorted by name; warp-error-ssim x100 with 2
    decimals, everything else with 4.  Returns the text of result.txt."""
    lines = [f"{name} - {prompt}"]
    for metric, score in sorted(scores.items()):
        if "warp-error-l1" in metric:
            lines.append(f"{metric}: {score * 1e5:.2f}")
        elif "warp-error-l2" in metric or "warp-error-ssim" in metric:
            lines.append(f"{metric}: {score * 100:.2f}")
        else:
            lines.append(f"{metric}: {score:.4f}")
    return "\n".join(lines) + "\n"
