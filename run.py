"""Entry point with the reference's surface (run.py:8-32): python run.py --config Y | -i video -p prompt [-n neg] [--multi_axis],
plus [--light left|right|top|bottom|source] [--strength F]: IC-Light's "Lighting Preference" start (generation.init_latent / init_strength),
[--iclight_model fc|fbc] [--bg_source upload|upload_flip|left|right|top|bottom|grey]: IC-Light's background-conditioned model
(generation.iclight_model / bg_source / fbc_matting; models.iclight_offset is then the fbc file) -- the UNet sees the foreground and a background latent,
and [--highres_scale F] [--highres_denoise F]: IC-Light's highres pass (generation.highres_scale / highres_denoise) -- the relit frames are resized
with PIL's LANCZOS filter to multiples of 64 and refined by a second img2img denoise; flows, masks, ids, output_gt and the result live at that size.
[--light_sweep A0 A1] (generation.light_path: keyframes [[pos, angle_deg], ...]): an animated light -- every frame gets a ramp at its own angle (the
side the light comes FROM: 0 left, 90 top, 180 right, 270 bottom), the img2img start under fc (with --strength), the background under fbc.
[--normal]: IC-Light's "Compute Normal" on the fbc model (generation.normal) -- four relights under the left / right / bottom / top ramps with one seed
become normal.npy / normal.mp4 (per-frame surface normals), relit_<side>.npy and the ambient video as output.*; no stage 1 / 2.
[--prompt_sweep PROMPT_A PROMPT_B] (generation.prompt_path: keyframes [[pos, "prompt"], ...]): a prompt that changes over the clip -- every frame's text
conditioning of the xy passes is the blend of its two neighbouring keyframes' embeddings; -p / generation.prompt still names the run.
[--ip_image PATH] [--ip_scale S] (generation.ip_adapter: {image, scale, path}): IP-Adapter -- the relight is steered towards a reference photograph;
its CLIP ViT-H/14 embedding (models.image_encoder) becomes 4 image tokens every text cross-attention of the xy passes also attends to (models.ip_adapter).
[--detail [SIGMA]] [--detail_mode add|ratio] [--detail_blend B] (generation.detail_transfer: {sigma, mode, blend, channels}): detail transfer -- the last
step gives the relit frames the source's high frequencies (texture, small text, faces) back and keeps the relight's low ones (the new light).
[--keyframes K] (generation.keyframes: K or {interval, alpha, diff_threshold, eps}): keyframe relighting -- only every K-th frame is denoised; the frames
in between are their source frame times the two neighbouring keys' gain field relit / source, carried along the chained flows; stage 1 / 2 see all frames.
[--noise_mode same|vanilla|warp] [--noise_warp_steps 0|1] (generation.noise_mode / noise_warp: {steps}): warp carries the noise from frame to frame
along the backward optical flow -- the start noise and, with steps on (the default), the per-step noise of the SDE solver.
[--fullres [RADIUS]] [--fullres_eps E] [--fullres_guide rgb|luma] (generation.fullres: true, a radius or {radius, eps, guide}): full-resolution output
-- the very last step fits relit ~ a * source + b at the size of the result (a guided filter), upsamples the smooth fields a, b and applies them to the
source's native pixels: output_fullres.npy / output_fullres.* at the source's own resolution beside output.*, which stay what they were.
data.scene_type picks the parser (generate.py:84-95): video (VideoDataParser) or sceneflow (SceneFlowDataParser: ground-truth depth, poses and
flows -> voxelised Unique Video Tensor ids); carla and interiornet are not built.

load_config -> seed_everything -> init_iclight (generation.use_lora: the LoRA of generation.lora merged into the UNet and the text encoder) ->
Generator (start latents from generation.latents_path when an inversion saved them) -> output.mp4 (frames / .npy when the image has no encoder), output_gt, loss
curves and config.yaml with the reference's metric keys (total_time, sec_per_frame, max_memory_allocated, total_number_of_frames;
generate.py:607-630).
Multi-GPU: torchrun --nproc-per-node N run.py ... shards frames over the ranks (tc_light_amd/parallel.py).
"""
import os
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # RCCL between processes needs dmabuf IPC on this driver (set before HIP starts)
import random
import sys
from types import SimpleNamespace

import numpy as np
import torch

from tc_light_amd.config_utils import Config, load_config, save_config
from tc_light_amd.dataparser import VideoDataParser, get_frame_ids, save_loss_curve, save_video
from tc_light_amd.generate import DEFAULTS, Generator
from tc_light_amd.hostlogic import (RESOLVED_KEYS, check_detail, check_highres_tokens, check_ip_adapter, cond_channels, fbc_background_per_frame,
                                    highres_size, keyframe_ids, light_angles, prompt_table, resolve_generation)
from tc_light_amd.model_utils import allow_random, init_iclight
from tc_light_amd.parallel import Dist
from tc_light_amd.text import encode_prompt_pair, encode_prompt_set


def seed_everything(seed):
    torch.manual_seed(seed); torch.cuda.manual_seed_all(seed); random.seed(seed); np.random.seed(seed)


def resolve_options(config):
    """Everything the configuration alone decides, refused here when malformed or unsupported: before a model is loaded, the video read or flows
    estimated.  The normalised generation.* values are written back (config.yaml records them).  -> what the run is: scene_type, fbc / light / normal /
    highres, data_hr (the data section at the final size of the highres pass), the LoRA and the IP-Adapter block."""
    g = config.generation
    if config.sd_version != "iclight":
        raise NotImplementedError("tc_light_amd implements the IC-Light path (sd_version: iclight); see invert.py")
    if g.prompt is None:
        raise NotImplementedError("generation.prompt is null: the Cosmos/Pixtral prompt up-sampler (generate.py:538-549) is outside this "
                                  "engine -- give a prompt (-p ... or generation.prompt)")
    scene_type = str(config.data.get("scene_type", "video")).lower()      # generate.py:84-95
    if scene_type in ("carla", "interiornet"):
        raise NotImplementedError(f"data.scene_type '{scene_type}': this dataparser is not yet built in tc_light_amd (video and sceneflow are)")
    if scene_type not in ("video", "sceneflow"):
        raise NotImplementedError(f"Scene type '{scene_type}' is not supported.")
    opts = {**DEFAULTS, **g, **config.post_opt}
    opts["fbc_matting"] = bool(opts["fbc_matting"])
    opts["scene_type"] = scene_type       # generation.keyframes is refused beside sceneflow
    # init_latent, the highres pass, fbc, light_path, normal, prompt_path, keyframes, noise_mode warp: each refused by the names of its keys
    r = resolve_generation(opts)
    g.update({k: r[k] for k in RESOLVED_KEYS}, fbc_matting=opts["fbc_matting"], normal=opts["normal"])
    o = SimpleNamespace(scene_type=scene_type, fbc=r["fbc"], light=r["light"], normal=bool(r["normal_sides"]), highres=r["highres"], data_hr=None,
                        lora=None, keyframes=r.get("keyframes"))      # the normalised block; None when off (interval 1 included)
    g.keyframes = None if o.keyframes is None else Config(o.keyframes)      # what config.yaml records
    o.noise_warp = r.get("noise_warp")        # the normalised block under noise_mode warp, else None
    if o.noise_warp is not None:
        g.noise_warp = Config(o.noise_warp)
    o.fullres = r.get("fullres")              # the normalised block; None when off
    g.fullres = None if o.fullres is None else Config(o.fullres)
    if o.normal:
        print("[INFO] generation.normal: the four ramps left / right / bottom / top are the backgrounds; generation.bg_source and "
              "generation.background_image_path are not consulted.")
        if opts["apply_opt"]:
            print("[INFO] generation.normal: stage 1 / 2 do not run on the four relights and no flows are estimated (exposure alignment per direction "
                  "would bias their ratios); post_opt.apply_opt is recorded as false.")
        config.post_opt.apply_opt = False
    if g.prompt_path is not None:
        print("[INFO] generation.prompt_path: the xy passes are conditioned on the keyframe prompts, blended per frame; generation.prompt names the "
              "run and is recorded in config.yaml, it conditions nothing.  negative_prompt, prompt_t and negative_prompt_t are used as they are.")
    # IP-Adapter (generation.ip_adapter; --ip_image / --ip_scale): a malformed block, a missing image, generation.normal beside it and missing weight
    # files (models.ip_adapter, models.image_encoder; unless allow_random) are refused too
    models = config.get("models") or {}
    o.ip_block = check_ip_adapter(opts["ip_adapter"], g.normal, models, allow_random(models))
    if o.ip_block is not None:
        g.ip_adapter = Config({k: o.ip_block[k] for k in ("image", "scale", "path")})      # what config.yaml records
    # detail transfer (generation.detail_transfer; --detail / --detail_mode / --detail_blend): a malformed block, generation.normal beside it and fbc
    # without its matte are refused too; the normalised block is what config.yaml records
    o.detail = check_detail(opts["detail_transfer"], normal=bool(g.normal), iclight_model=r["iclight_model"], fbc_matting=opts["fbc_matting"])
    if o.detail is not None:
        g.detail_transfer = Config(o.detail)
    if o.light and o.fbc:
        print("[INFO] generation.light_path: the per-frame ramps are the backgrounds; generation.background_image_path is not consulted.")
    o.upload = o.fbc and not o.normal and not o.light and g.bg_source in ("upload", "upload_flip")      # fbc is conditioned on a background file
    if o.upload and not g.get("background_image_path"):
        raise ValueError(f"generation.bg_source {g.bg_source} needs generation.background_image_path")
    if o.highres:     # the final size; the producers (flows, masks, ids) and output_gt live there, so a second parser is built at that size
        H2, W2 = highres_size(config.data["height"], config.data["width"], g.highres_scale)
        check_highres_tokens(H2, W2, opts["chunk_size"])
        o.data_hr = Config(dict(config.data, height=H2, width=W2))
    if g.get("use_lora"):             # generate_utils.py:95-96; the file is read and its layout checked here
        from tc_light_amd.lora import from_config
        o.lora = from_config(g.get("lora"))
    return o


def setup_device():
    """This process's device and its place among the ranks (torchrun's environment); more than one rank: the process group."""
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl", device_id=dev)
    return dev, Dist(rank, world)


def load_frames(config, o, dev):
    """-> the clip: parser, parser_hr (where stage 1 / 2 run: the second parser at the final size under the highres pass, else the same), frame_ids,
    frames (all frames at the working size) and frames_out (the source frames at the size of the result)."""
    if o.scene_type == "sceneflow":
        from tc_light_amd.sceneflow import SceneFlowDataParser
        parser = SceneFlowDataParser(config.data, dev)
    else:
        parser = VideoDataParser(config.data, dev)
    parser_hr = type(parser)(o.data_hr, dev) if o.highres else parser
    g = config.generation
    frame_ids = get_frame_ids(g.frame_range, parser.n_frames, g.frame_ids)
    config.total_number_of_frames = len(frame_ids)
    frames = frames_out = parser.load_video(frame_ids)
    if o.highres:
        if o.scene_type == "video":
            parser_hr._all = parser._all          # the clip is read once
        frames_out = parser_hr.load_video(frame_ids)
    if o.fullres is not None:                 # refused here, with the sizes, when the source is no larger than the result
        from tc_light_amd.fullres import geometry
        o.fullres_geo = geometry(*parser.native_size(), parser_hr.h, parser_hr.w)
        g.fullres_size = [o.fullres_geo["Hc"], o.fullres_geo["Wc"]]
    return SimpleNamespace(parser=parser, parser_hr=parser_hr, frame_ids=frame_ids, frames=frames, frames_out=frames_out)


def load_flows(config, o, clip, models, dev, d):
    """The stage-1 / 2 producers' input -> (flows, scene), both None without post_opt.apply_opt -- unless generation.keyframes is on: propagation
    needs the flows of the whole clip even without the optimiser; so does generation.noise_mode warp, which carries the noise along them.  sceneflow: every rank reads the files itself --
    ground-truth (or RAFT) flows, masks and the voxelised ids all come from load_data.  video: rank 0 owns the flow cache (read, or estimated with
    MemFlowNet / RAFT (data.flow_model) and written: video_dataparser.py:63-110); the other ranks receive the tensors.  A failure on rank 0 (e.g.
    missing MemFlow weights) is announced before the payload so that every rank raises instead of waiting in the broadcast until the collective
    times out."""
    if not config.post_opt.apply_opt and o.keyframes is None and o.noise_warp is None:
        return None, None
    ok_random, frame_ids, parser_hr = allow_random(models), clip.frame_ids, clip.parser_hr
    if o.scene_type == "sceneflow":
        return None, parser_hr.load_data(frame_ids, models=models, allow_random=ok_random)
    flows = err = None
    if d.rank == 0:
        try:
            # the on-disk cache belongs to the working size: with the highres pass on it is neither read nor written
            flows = None if o.highres else clip.parser.load_flow_cache(frame_ids)
            if flows is None:
                flows = parser_hr.estimate_and_cache_flow(clip.frames_out, frame_ids, parser_hr.make_flow_engine(models, ok_random),
                                                          save_flow=not o.highres)
        except Exception as e:            # noqa: BLE001 - re-raised below on every rank
            err = e
    if d.world > 1:
        ok = torch.tensor([0 if err is not None else 1], device=dev)
        torch.distributed.broadcast(ok, src=0)
        if int(ok.item()) == 0:
            torch.distributed.destroy_process_group()
            raise err if err is not None else RuntimeError("rank 0 failed to load / estimate the optical flow (see its traceback)")
        flows = flows if d.rank == 0 else tuple(torch.empty(len(frame_ids), 2, parser_hr.h, parser_hr.w, device=dev) for _ in range(2))
        for t in flows:
            torch.distributed.broadcast(t, src=0)
    elif err is not None:
        raise err
    return flows, None


def load_background(config, o, clip, models, dev, d, kf_ids=None):
    """-> (rmbg, background, bg_per_frame): the matting engine where it is needed (background compositing, generate.py:68-69, 147-167; fbc: the alpha
    of the grey matte), and this rank's frames of generation.background_image_path -- composited behind the foreground (background_cond), or the
    background the fbc model is conditioned on: one frame for all, or one per frame (bg_per_frame, the same answer on every rank).
    kf_ids (generation.keyframes): the frames that are denoised -- a per-frame background is indexed by them before the ranks take their blocks."""
    g, n = config.generation, len(clip.frame_ids)
    lo, hi = d.range(n if kf_ids is None else len(kf_ids))
    pick = lambda b: b if kf_ids is None else b[kf_ids]
    rmbg = background = bg_per_frame = None
    if g.get("background_cond") or (o.fbc and g.fbc_matting):
        from tc_light_amd.model_utils import load_rmbg_state
        from tc_light_amd.rmbg import RMBGEngine
        rmbg = RMBGEngine(load_rmbg_state(models.get("rmbg"), allow=allow_random(models)), dev)
    if g.get("background_cond"):
        background = clip.parser.load_video(path=g.background_image_path)
        if background.shape[0] == n:                     # a per-frame background video: this rank's block of it
            background = pick(background)
            if d.world > 1:
                background = background[lo:hi]
    elif o.upload:
        background = clip.parser.load_video(path=g.background_image_path)
        bg_per_frame = fbc_background_per_frame(background.shape[0], n, g.bg_source)
        if bg_per_frame:
            background = pick(background)
            if d.world > 1:
                background = background[lo:hi]
    return rmbg, background, bg_per_frame


def save_run(config, name, info, out, clip, first=None, then=None):
    """What every run directory holds, rank 0 only: the time and memory bookkeeping, config.yaml with the reference's metric keys, output.npy --
    written before anything that needs an encoder, so it survives whatever fails behind it -- output.* and output_gt.* (generate.py:613-630).
    first(path) runs before all of it, then(path) between output.npy and the videos.  -> the directory."""
    g, n, fps = config.generation, len(clip.frame_ids), clip.parser.fps
    config.total_time += info["total_time"]
    config.sec_per_frame = config.total_time / n
    config.max_memory_allocated = max(config.max_memory_allocated, info["max_memory_allocated"])
    g.scheduler_steps, g.steps_executed = info["scheduler_steps"], info["steps_executed"]
    path = os.path.join(g.output_path, f"lmr_{g.local_merge_ratio}_gmr_{g.global_merge_ratio}_alpha_t_{g.alpha_t}_opt_{name}")
    os.makedirs(path, exist_ok=True)
    if first is not None:
        first(path)
    save_config(config, path, gene=True)
    out = out.clamp(0, 1)
    np.save(os.path.join(path, "output.npy"), (out * 255).byte().permute(0, 2, 3, 1).cpu().numpy())
    if then is not None:
        then(path)
    save_video(out, path, save_frame=bool(g.get("save_frame", False)), fps=fps, gif=False)
    gt_path = os.path.join(path, "gt")
    if not os.path.exists(gt_path) or len(os.listdir(gt_path)) != n:
        save_video(clip.frames_out, path, save_frame=False, post_fix="_gt", fps=fps, gif=False)
    return path


def save_normal_run(config, name, nrm, ambient, relit, info, clip):
    """The run directory of generation.normal: normal.npy first (u8 [N,H,W,3], RGB = (u, v, h)), then relit_<side>.npy and normal.mp4 beside the
    ambient video as output.* and output_gt.* (what evaluate.py looks for)."""
    config.generation.normal_denoise_seconds = {s: float(t) for s, t in info["denoise_per_direction"].items()}

    def sides(path):
        for side, frames in relit.items():
            np.save(os.path.join(path, f"relit_{side}.npy"), (frames.clamp(0, 1) * 255).byte().permute(0, 2, 3, 1).cpu().numpy())
        # save_video quantises trunc(255 x): (u + 0.5)/255 comes back as u whatever the rounding of the division
        save_video((nrm.permute(0, 3, 1, 2).float() + 0.5) / 255, path, save_frame=False, stem="normal", fps=clip.parser.fps, gif=False)
    path = save_run(config, name, info, ambient, clip, first=lambda p: np.save(os.path.join(p, "normal.npy"), nrm.cpu().numpy()), then=sides)
    print(f"[INFO] normals of {len(clip.frame_ids)} frames (4 relights each) in {info['total_time']:.1f} s "
          f"({1 / config.sec_per_frame:.3f} frames/s) -> {path}")


def save_relit_run(config, o, name, out, info, clip):
    """The run directory of a relight: what the run was (light_path, the highres pass) recorded in config.yaml, and the loss curves of stage 1 / 2."""
    g, n = config.generation, len(clip.frame_ids)
    if o.light:                               # light_path is in g already; the angles of the first and the last frame of the run
        g.light_angle_first, g.light_angle_last = (float(a) for a in light_angles(g.light_path, [0.0, 1.0 if n > 1 else 0.0]))
    if "keyframes" in info:                   # the block is in g already; how many frames went through the denoise, the share of hole pixels
        g.keyframes_denoised, g.keyframes_holes = int(info["keyframes"]["denoised"]), float(info["keyframes"]["holes"])
    if o.highres:                             # total_time / sec_per_frame cover both passes
        g.highres_size = list(info["highres_size"])
        g.highres_scheduler_steps, g.highres_steps_executed = info["highres_scheduler_steps"], info["highres_steps_executed"]

    def curves(path):
        if config.post_opt.apply_opt:
            save_loss_curve(info["losses_exposure"], path, "loss_exposure")
            if info["losses_unique"] is not None:
                save_loss_curve(info["losses_unique"], path, "loss_unique_tensor")
    path = save_run(config, name, info, out, clip, then=curves)
    print(f"[INFO] {n} frames in {info['total_time']:.1f} s ({1 / config.sec_per_frame:.3f} frames/s) -> {path}")
    return path


def save_fullres(config, o, path, out, clip):
    """generation.fullres, the very last step, rank 0 only (frames are independent; sharding them over the ranks is not built): the relight applied
    to the source's native pixels.  The fit is made against what output.npy holds -- the result quantised to uint8 -- and the source frames at that
    size, so output_fullres.* is a function of the run's written output and its source alone.  -> output_fullres.npy (uint8 [N,Hc,Wc,3]) and the
    video of the same stem."""
    from tc_light_amd.fullres import fullres
    geo, b = o.fullres_geo, o.fullres
    relit = (out.clamp(0, 1) * 255).byte().float() / 255.0
    native = clip.parser.native_u8(clip.frame_ids)
    full = fullres(clip.frames_out.float().contiguous(), relit.contiguous(), native, b["radius"], b["eps"], b["guide"],
                   crop=(geo["Y0"], geo["X0"], geo["Hc"], geo["Wc"]))
    np.save(os.path.join(path, "output_fullres.npy"), full.numpy())
    # save_video quantises trunc(255 x): (u + 0.5) / 255 comes back as u whatever the rounding of the division
    save_video((full.permute(0, 3, 1, 2).float() + 0.5) / 255, path, save_frame=False, stem="output_fullres", fps=clip.parser.fps, gif=False)
    print(f"[INFO] generation.fullres: {full.shape[0]} frames of {geo['Hc']}x{geo['Wc']} -> {os.path.join(path, 'output_fullres.npy')}")


def main(argv=None):
    config = load_config(argv)
    seed_everything(config.seed)
    o = resolve_options(config)               # before any model
    dev, d = setup_device()
    models = config.get("models") or {}
    ok_random = allow_random(models)
    pipe, scheduler, config.model_key = init_iclight(dev, models, seed=config.seed, lora=o.lora,
                                                     cond_channels=cond_channels(config.generation.iclight_model))
    config.max_memory_allocated, config.total_time = 0, 0
    clip = load_frames(config, o, dev)
    flows, scene = load_flows(config, o, clip, models, dev, d)
    g, n = config.generation, len(clip.frame_ids)
    # generation.keyframes: only the key frames are denoised -- the frames, backgrounds and start latents handed to the generator are theirs
    kf_ids = None if o.keyframes is None else keyframe_ids(n, o.keyframes["interval"])
    rmbg, background, bg_per_frame = load_background(config, o, clip, models, dev, d, kf_ids)
    n_gen = n if kf_ids is None else len(kf_ids)
    frames_in = clip.frames if kf_ids is None else clip.frames[kf_ids]
    frames_hr = None if not o.highres else (clip.frames_out if kf_ids is None else clip.frames_out[kf_ids])
    lo, hi = d.range(n_gen)
    cfg = dict(g); cfg.update(config.post_opt); cfg["seed"] = config.seed
    # generation.latents_path: which saved start latents are this run's
    cfg["frame_ids"] = clip.frame_ids if kf_ids is None else [clip.frame_ids[k] for k in kf_ids]
    cfg["model_key"] = config.model_key
    image_prompt = None
    if o.ip_block is not None:    # on every rank, once per run: the image tower is built, run on the one image and freed before the UNet loop
        from tc_light_amd import ip_adapter
        image_prompt = ip_adapter.build(o.ip_block, dev, allow=ok_random)
    gen = Generator(pipe.unet, pipe.vae, cfg, dist=d, scheduler=scheduler, rmbg=rmbg, image_prompt=image_prompt)
    text = dict(allow_random=ok_random, lora=o.lora)
    for name, prompt in g.prompt.items():
        if g.prompt_path is not None:      # every distinct keyframe prompt is encoded once; the rows of this rank's frames are blended from them
            uncond, keys = encode_prompt_set(prompt_table(g.prompt_path, n)[0], g.negative_prompt, dev, models.get("text_encoder"), **text)
            conds = gen.frame_text(uncond, keys, hi - lo, n_total=n)      # (refused beside generation.keyframes: n is every frame)
        else:
            conds = encode_prompt_pair(prompt, g.negative_prompt, dev, models.get("text_encoder"), **text)
        conds_t = encode_prompt_pair(g.prompt_t, g.negative_prompt_t, dev, models.get("text_encoder"), **text)
        if o.normal:
            nrm, ambient, relit, info = gen.normals(clip.frames[lo:hi], conds, conds_t, n_total=n)
            if d.rank == 0:
                save_normal_run(config, name, nrm, ambient, relit, info, clip)
            continue
        masks = inv = k = past = None
        if scene is not None:
            masks, inv, k, past = scene["masks"], scene["inv"], scene["k"], scene["past_flows"]
        elif config.post_opt.apply_opt:
            from tc_light_amd.flow_ids import soft_masks_and_ids
            fut, past = flows
            masks, inv, k = soft_masks_and_ids(clip.frames_out, fut, past, alpha=clip.parser.alpha)
        elif o.noise_warp is not None:        # no optimiser, so no track ids: the masks alone, which the noise is carried under
            from tc_light_amd.flow_ids import get_soft_mask_bwds
            fut, past = flows
            masks = get_soft_mask_bwds(clip.frames_out, fut, past, alpha=clip.parser.alpha)
        out, info = gen(frames_in[lo:hi], conds, conds_t, past, masks, inv, n_total=n_gen, k=k, background=background,
                        frames_hr=frames_hr[lo:hi] if o.highres else None, background_per_frame=bg_per_frame,
                        source=clip.frames_out if o.detail is not None or kf_ids is not None else None,
                        flows=flows if kf_ids is not None else None, keyframes=kf_ids)
        if d.rank == 0:
            path = save_relit_run(config, o, name, out, info, clip)
            if o.fullres is not None:
                save_fullres(config, o, path, out, clip)
    if d.world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
