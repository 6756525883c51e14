"""TC-Light pipeline driver on the MI355X engine -- host-side mirror of generate.py::Generator (reference).

  prepare_data -> _prepare_prompts_and_conditions -> ddim_sample{pred_noise per xy-chunk; temporal_denoise (yt-plane);
  scheduler.step} -> decode_latents_batch -> exposure_align -> unique_tensor_optimization        (generate.py:560-611)
Generator.__call__: prepare_data, encode_conds and (img2img) build_start -> ddim_sample -> optional highres_pass -> decode_gather -> post_optimize.
What each option adds to that is said at its key in DEFAULTS; hostlogic.resolve_generation checks and resolves them all, once.  Generator.normals
(generation.normal) runs ddim_sample and the decode once per ramp from the same start and one tcl_fbc_normal launch over the four results.

Python sequences kernel launches and collectives; tensors never leave the device inside the timed region and there is no
per-iteration host sync (the reference syncs on loss.item() and moves the token bank through the CPU).
"""
import math
import os
import struct
import time
from types import SimpleNamespace

import numpy as np
import torch

from .lib import lib, stream
from . import hostlogic as HL
from . import post_opt
from .dataparser import check_latent_exists, get_latents_dir, load_latent
from .parallel import Dist, sharded_temporal_pass
from .scheduler import DPMSolverSDEScheduler
from .unet import FrameText

H16 = torch.float16
I32 = torch.int32

DEFAULTS = dict(  # configs/tclight_default.yaml (generation / post_opt sections)
    guidance_scale=2.0, n_timesteps=25, chunk_size=4, chunk_ord="mix-4", local_merge_ratio=0.6, merge_global=True,
    global_merge_ratio=0.5, global_rand=0.5, align_batch=True, max_downsample=2, noise_mode="same", alpha_t=0.0,
    final_factor_t=0.01, win_size_t=64, apply_opt=True, epochs_exposure=35, epochs=70, batch_size=16, lambda_dssim=0.2,
    lambda_flow=0.8, lambda_tv=0.05, feature_lr=0.05, exposure_lr_init=0.01, exposure_lr_final=0.001, seed=12345,
    post_opt_mode="replicated",      # multi-GPU only: how stage 1 / stage 2 run once the decoded frames are all-gathered.
                                     # "replicated" (default): every rank runs stage 2 in full on all frames, no collective (path 2 is
                                     #   bit-reproducible, so the replicas agree bit for bit); stage 1 is dealt over the ranks, its only exchange
                                     #   the [N,3,4] gradient.  "replicated_all": stage 1 replicated too -- the one-GPU result, bit for bit.
                                     # "global": ONE parameter set with the mini-batch dealt over the ranks, gradients meet in all_reduce /
                                     #   reduce_scatter (kept for memory-bound cases).  "shard": each rank's frame block as a video of its own
                                     #   (tracks cut at the block seams) -- NOT the reference's result.
    shard_post_opt=False,            # legacy spelling of post_opt_mode="shard"
    latents_path=None, model_key="iclight", frame_ids=None,
    # ^ generation.latents_path (generate.py:563-566): saved start latents `<latents_path>/<model_key>/noisy_latents_<first timestep>.pt`, a tensor
    #   over the video's frames of which `frame_ids` (None: all) are this run's; when the file exists it replaces the random start noise.
    highres_scale=1.0, highres_denoise=0.5,
    # ^ IC-Light's highres pass (gradio_demo_iclight.py:301-334): scale in [1, 3], 1.0 = off (the demo always runs it; here the default leaves every
    #   path, RNG draw and output bit as it was).  On: the relit frames are decoded, quantised to u8, resized with PIL's LANCZOS filter to
    #   HL.highres_size (multiples of 64), encoded again and refined by a second img2img denoise of strength highres_denoise at that size; stage 1 / 2
    #   run at the final size, so the caller hands flows, masks and ids of that size and the source frames at both sizes.
    init_latent="none", init_strength=0.9,
    # ^ IC-Light's "Lighting Preference" (gradio_demo_iclight.py:235-299: bg_source, lowres_denoise): left | right | top | bottom start the denoise from
    #   the VAE latent of a light gradient, `source` from the frames' own clean latents, noised to init_strength -- the scheduler is set to
    #   round(n_timesteps / init_strength) steps and entered at the index that leaves int(steps * init_strength) of them (HL.img2img_schedule).
    #   "none": the start is noise (or latents_path) and init_strength changes nothing.  Otherwise latents_path is not consulted.
    iclight_model="fc", bg_source="upload", fbc_matting=True,
    # ^ IC-Light's second model, iclight_sd15_fbc (utils/model_utils.py:97-179, init_iclight_bg): "fbc" conditions the 12-channel UNet on the
    #   foreground latent AND a background latent, the background being the lighting condition.  bg_source: upload | upload_flip (the frames handed
    #   in as `background`, as they are or mirrored) | left | right | top | bottom | grey (a ramp or a flat grey built on the device, HL.BG_RAMPS).
    #   fbc_matting: the foreground is matted onto 127-grey with BriaRMBG's alpha before it is encoded (the background demo's run_rmbg); false feeds
    #   the frames as they are and needs no RMBGEngine.  "fc" (default): none of this is consulted and every path is bit for bit what it was.
    light_path=None,
    # ^ an animated light: keyframes [[pos, angle_deg], ...] over the clip (pos 0 .. 1, frame i of N at i/(N - 1); the angle is the side the light comes
    #   FROM: 0 left, 90 top, 180 right, 270 bottom; linear in the angle, several turns allowed).  Every frame gets its own ramp (light_ramps): under fc
    #   it is the img2img start of that frame, with init_strength exactly as init_latent uses it (init_latent itself stays none); under fbc it is that
    #   frame's background (bg_source stays at its default).  None (default): nothing of it is consulted and every path is what it was.
    normal=False,
    # ^ IC-Light's "Compute Normal" (the background demo's process_normal), fbc only: Generator.normals relights the frames under the left / right /
    #   bottom / top ramps from one seed and turns the four results into per-frame surface normals and the ambient image (tcl_fbc_normal).
    #   bg_source is not consulted, stage 1 / 2 do not run.  false (default): nothing of it is consulted and every path is what it was.
    prompt_path=None,
    # ^ a prompt that changes over the clip: keyframes [[pos, "prompt"], ...] (pos as in light_path, strictly increasing, 0 first and 1 last).  Every
    #   frame's text conditioning of the xy passes is the linear blend of its two neighbouring keyframes' embeddings (frame_text); the negative prompt
    #   is one for all, the yt passes keep prompt_t.  generation.prompt is then only the run's name.  None (default): nothing of it is consulted and
    #   every path is what it was.  With it the K / V panels of the distinct rows stay resident (UNetEngine.text_rows_bytes: 7.6 MB per row over
    #   the 16 blocks, 2.3 GB for 300 distinct rows); the token budget below is taken from what is left.
    ip_adapter=None,
    # ^ IP-Adapter: relight towards a reference image.  {image: <path>, scale: <float in [0, 2]>, path: <adapter file, default models.ip_adapter>}
    #   (HL.check_ip_adapter); the image goes once through the CLIP ViT-H/14 image tower (models.image_encoder) and the adapter's projection to 4
    #   tokens, and every text cross-attention of the xy passes -- the highres refine included -- adds scale * Attention(q, K_ip, V_ip)
    #   (tcl_attention_ip_add_f16); the yt passes do not (a y-t slice is not an image the photograph describes).  The Generator takes the tokens as
    #   image_prompt= (ip_adapter.build).  None (default): nothing of it is consulted and every path is what it was.
    detail_transfer=None,
    # ^ detail transfer: {sigma, mode: add | ratio, blend, channels: rgb | luma} or a bare sigma (HL.check_detail).  The last step of __call__, behind
    #   stage 1 / 2: the returned frames keep their low frequencies (the new light) and take the high ones (texture, small text, faces) from the source
    #   frames handed in as source= -- one tcl_detail_transfer_f32 call over all frames (detail.py), weighted by the matting alpha under fbc.
    #   None (default): nothing of it is consulted and every path is what it was.
    keyframes=None,
    # ^ keyframe relighting: an integer K or {interval: K, alpha, diff_threshold, eps} (HL.check_keyframes).  Only every K-th frame (HL.keyframe_ids) is
    #   handed in and denoised; propagate_step, behind the decode and the highres pass and in front of stage 1 / 2, fills the frames in between: their
    #   source frame times the gain field relit / source of the two neighbouring keys, carried along the chained flows handed in as flows= and blended
    #   by distance (keyframe.py: tcl_flow_chain_f32, tcl_keyframe_propagate_f32).  Stage 1 / 2 and detail_transfer then see all frames.
    #   None (default) or interval 1: nothing of it is consulted and every path is what it was.
    noise_warp=None,
    # ^ read under noise_mode warp only: {steps: <bool>} (HL.check_noise_warp; default {steps: true}).  noise_mode warp: the start noise is carried
    #   from frame to frame along the backward flows handed to __call__ as past_flows / mask_bwds -- a pixel-resolution field, the same where nothing
    #   moves, following the surface where it moves, fresh where something is uncovered, white and unit-variance in every frame (noisewarp.py:
    #   tcl_noise_warp_count, tcl_noise_warp_apply_f32); steps: the per-step noise of the SDE solver is a new chain over the same flows too.
    #   noise_mode same | vanilla: nothing of it is consulted and every path, launch and draw is what it was.
    fullres=None,
    # ^ full-resolution output: true, a radius or {radius, eps, guide: rgb | luma} (HL.check_fullres).  Not a step of the Generator: run.py, behind
    #   everything else, fits relit ~ a * source + b at the size of the result and applies the upsampled fields to the source's native pixels
    #   (fullres.py: tcl_guided_fit_f32, tcl_guided_apply_u8) -> output_fullres.*.  The Generator only checks the key with the others.
    #   None (default): nothing of it is consulted and every path is what it was.
    max_tokens_per_pass=None)
    # ^ level-0 tokens (samples x pixels) one block-major UNet pass may carry; longer chunk lists are split into consecutive groups.  None:
    #   TCL_MAX_TOKENS_PER_PASS (read when the Generator is built), else min(16 M, 80 % of the device's free memory / 10.5 KB) -- a pass peaks at
    #   ~10.4 KB of activations per token (90 GB for the 8.64 M tokens of 300 frames at 1280x720).  16 M is the whole xy step of 555 frames at
    #   1280x720 in ONE pass: one group is faster than several and its GEMM shapes do not depend on the random chunk lengths.
    #   tests/test_gpu_fullsize.py pins pass-size invariance (same bits) beyond 2^31 elements.


def default_max_tokens_per_pass(unet, dev, reserve=0):
    """max_tokens_per_pass when the configuration leaves it open (see DEFAULTS): TCL_MAX_TOKENS_PER_PASS, else what the device's free memory carries.
    reserve: bytes that will be held beside the pass and are not allocated yet (the per-frame text K / V panels of generation.prompt_path)."""
    env = os.environ.get("TCL_MAX_TOKENS_PER_PASS")
    if env:
        return int(env)
    free = 288 << 30
    if torch.cuda.is_available() and dev.type == "cuda":      # the driver's free bytes + what this process's caching allocator holds unused
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if hasattr(unet, "panel_cache_cap"):      # persistent attention panels live beside the pass (a stand-in engine keeps none)
        free -= max(0, unet.panel_cache_cap() - unet.panel_cache_bytes())
    free -= int(reserve)
    return int(min(16_000_000, max(1_000_000, 0.8 * free / 10_500)))


class Generator:
    def __init__(self, unet, vae, config=None, dist=None, scheduler=None, rmbg=None, image_prompt=None):
        cfg = dict(DEFAULTS)
        cfg.update(config or {})
        r = HL.resolve_generation(cfg)     # every option checked once, in run.py's order; what is refused is refused before anything is built
        cfg.update({k: r[k] for k in HL.RESOLVED_KEYS})
        cfg["keyframes"] = r.get("keyframes")      # the normalised block, None when off (interval 1 included)
        cfg["noise_warp"] = r.get("noise_warp")    # the normalised block, None unless noise_mode warp
        cfg["fullres"] = r.get("fullres")          # the normalised block, None when off; run.py's step, checked here with the others
        self.cfg = SimpleNamespace(**cfg)
        self.fbc, self.light, self.img2img, self.highres = r["fbc"], r["light"], r["img2img"], r["highres"]
        self.normal_sides = r["normal_sides"]                                      # () unless generation.normal
        # the caller's check, as check_ip_adapter is: not part of resolve_generation's result
        self.cfg.detail_transfer = HL.check_detail(cfg["detail_transfer"], normal=bool(cfg["normal"]), iclight_model=r["iclight_model"],
                                                   fbc_matting=cfg["fbc_matting"])
        self.schedule, self.schedule_highres = r["schedule"], r["schedule_highres"]      # (scheduler steps, begin index, steps executed)
        self.unet, self.vae, self.rmbg = unet, vae, rmbg
        self.dev = unet.dev
        self.L = lib()
        self.dist = dist or Dist()
        self.scheduler = scheduler or DPMSolverSDEScheduler()
        c = self.cfg
        # vidtome.apply_patch(...) (generate_utils.py:98-100); max_downsample is NOT forwarded by the reference (default 2)
        t = self.unet.tome
        t.args.update(local_merge_ratio=c.local_merge_ratio, merge_global=c.merge_global, global_merge_ratio=c.global_merge_ratio,
                      global_rand=c.global_rand, align_batch=bool(c.align_batch))
        if (c.ip_adapter is not None) != (image_prompt is not None):
            raise ValueError("generation.ip_adapter: the Generator takes the block's unet.ImagePrompt as image_prompt= (ip_adapter.build), and only then")
        if image_prompt is not None and c.normal:
            raise ValueError("generation.ip_adapter together with generation.normal is not supported")
        self.ip = image_prompt             # handed to every xy pass; the yt passes run without it
        self.n_total = None                # the run's frames over all ranks (_total); a caller may assign it before prepare_data
        self.bg_index = None               # fbc under light_path: the image of bg_frames that is each frame's background (None: bg_frames as they are)
        self._bg_per_frame = None          # fbc: is the background one frame per frame?  The entry point says (None: by the length of its latents)
        self.fbc_alpha = None              # fbc with matting: the alpha of this rank's frames (prepare_fbc), the weight of detail_transfer
        self.warp_flows = None             # noise_mode warp: (past_flows, mask_bwds) of ALL frames at the working size (prepare_start)
        cin = getattr(self.unet, "w", {}).get("conv_in", (None, None, None))[2]      # a stand-in engine may carry no weights
        if cin is not None and cin != 4 + HL.cond_channels(c.iclight_model):
            raise ValueError(f"generation.iclight_model {c.iclight_model}: the UNet's conv_in takes {cin} channels, expected "
                             f"{4 + HL.cond_channels(c.iclight_model)} (init_iclight(..., cond_channels={HL.cond_channels(c.iclight_model)}))")
        self._lanczos = {}                 # (in, out) -> device table of that axis
        self.batch_size = 2
        self.timing = {}
        if c.max_tokens_per_pass is None:
            reserve = 0
            if c.prompt_path is not None and c.frame_ids is not None and hasattr(self.unet, "text_rows_bytes"):
                # the K / V panels of the negative and of at most one row per frame of this rank (frame_ids unknown: the bound is not known here)
                lo, hi = self.dist.range(len(c.frame_ids))
                reserve = self.unet.text_rows_bytes(1 + hi - lo)
            c.max_tokens_per_pass = default_max_tokens_per_pass(self.unet, self.dev, reserve)

    # ------------------------------------------------------------------ data
    def prepare_data(self, frames, background=None, past_flows=None, mask_bwds=None):
        """frames: this rank's block [n_local,3,H,W] f32 in [0,1] on the device (generate.py:138-204).  background [1|n_local,3,H,W]:
        background compositing (generate.py:147-167): alpha from BriaRMBG on the resized frames, `alpha*fg + (1-alpha)*bg`.
        Under iclight_model fbc nothing is composited: prepare_fbc builds the two condition images and self.frames stays the source.
        past_flows / mask_bwds: the backward flows and masks of ALL frames, which noise_mode warp carries the noise along (prepare_start)."""
        c = self.cfg
        if self.fbc:
            self.prepare_fbc(frames, background)
        elif background is not None:
            if self.rmbg is None:
                raise RuntimeError("background compositing needs an RMBGEngine (Generator(..., rmbg=...))")
            alpha = self.rmbg.estimate_alpha(frames, self.batch_size)
            frames = alpha * frames + (1 - alpha) * background.to(frames)
        self.frames = frames.contiguous()
        self.prepare_start(frames.shape[0], *frames.shape[-2:], past_flows, mask_bwds)

    def prepare_start(self, n, H, W, past_flows=None, mask_bwds=None):
        """The start of one denoise of n local frames at (H, W): the device generator seeded afresh, then init_noise (or start_noise for an
        img2img start, or the saved latents of latents_path).  Generator.normals calls it once per direction, so all four start alike.
        noise_mode warp: past_flows [n_total,2,H,W] / mask_bwds [n_total,1,H,W] of all frames are checked and kept for the start and the steps."""
        c = self.cfg
        self.h, self.w = H // 8, W // 8
        self._total(n)
        self.warp_flows = None
        if c.noise_warp is not None:
            self.warp_flows = self._warp_inputs(past_flows, mask_bwds, 8 * self.h, 8 * self.w)
        self.rng_dev = torch.Generator(device=self.dev).manual_seed(int(c.seed))
        self.start_noise = None
        if self.img2img:
            if c.latents_path is not None:
                what = f"light_path {c.light_path}" if self.light else f"init_latent '{c.init_latent}'"
                print(f"[INFO] {what}: the start is built from it, generation.latents_path is not consulted.")
        elif c.latents_path is not None and self._load_start_latents(n):
            if c.noise_warp is not None:
                print("[INFO] noise_mode warp: the start comes from generation.latents_path; of the warped noise only generation.noise_warp.steps "
                      f"({'on' if c.noise_warp['steps'] else 'off'}) applies.")
            return
        z = self._draw_start(self.h, self.w)
        if self.img2img:
            self.start_noise = z           # f32: build_start adds it to x0
        else:                              # prepare_latents (generate.py:183-188); `same`: the one frame repeated
            self.init_noise = (z * self.scheduler.init_noise_sigma).to(H16).expand(n, -1, -1, -1).contiguous()

    def _total(self, n, n_total=None, keep=True):
        """The run's frames over all ranks, set here and nowhere else: what the caller says, else (keep) what is known already -- a caller may have
        assigned n_total -- else n local frames on every rank."""
        self.n_total = n_total or (self.n_total if keep else None) or n * self.dist.world
        return self.n_total

    def _now(self):
        """A timing point of __call__ / normals: the device drained, then the host clock."""
        torch.cuda.synchronize(self.dev)
        return time.perf_counter()

    def _draw_start(self, h, w):
        """z of one start at latent size (h, w), f32 from rng_dev.  noise_mode same: [1,4,h,w], one frame for all; vanilla: n_total frames are
        drawn and this rank's block is taken; warp: this rank's block of the chain over all n_total frames (_warp_chain)."""
        mode = self.cfg.noise_mode.lower()
        if mode == "same":
            return torch.randn(1, 4, h, w, generator=self.rng_dev, device=self.dev, dtype=torch.float32)
        if mode == "warp":
            lo, hi = self.dist.range(self.n_total)
            return self._warp_chain(h, w)[lo:hi]
        if mode != "vanilla":
            raise NotImplementedError(f"Noise mode '{self.cfg.noise_mode}' is not supported.")
        lo, hi = self.dist.range(self.n_total)
        return torch.randn(self.n_total, 4, h, w, generator=self.rng_dev, device=self.dev, dtype=torch.float32)[lo:hi]

    def _warp_inputs(self, past_flows, mask_bwds, H, W):
        """noise_mode warp: the flows and masks of all n_total frames at the working size, as noisewarp.warp_chain takes them."""
        shapes = [None if t is None else tuple(t.shape) for t in (past_flows, mask_bwds)]
        if shapes != [(self.n_total, 2, H, W), (self.n_total, 1, H, W)]:
            raise ValueError(f"generation.noise_mode warp: past_flows / mask_bwds {shapes}, expected {(self.n_total, 2, H, W)} and "
                             f"{(self.n_total, 1, H, W)} -- the backward flows and masks of ALL frames at the working size "
                             "(Generator(...)(frames, conds, conds_t, past_flows, mask_bwds, ...))")
        return past_flows.to(self.dev).float().contiguous(), mask_bwds.to(self.dev).float().contiguous()

    def _warp_chain(self, h, w):
        """noise_mode warp: one chain z [n_total,4,h,w] f32 over all frames from rng_dev -- one [4,8h,8w] draw per frame, in frame order, on every
        rank, so neither batching nor the number of ranks changes the stream."""
        from .noisewarp import field_draw, warp_chain
        if self.warp_flows is None:
            raise ValueError("generation.noise_mode warp: the backward flows and masks of all frames are missing (prepare_data(..., past_flows=, "
                             "mask_bwds=))")
        return warp_chain(field_draw(self.rng_dev, self.dev), *self.warp_flows, self.n_total, 8 * h, 8 * w)

    def _noised_start(self, n, x0, x0_stride, z, schedule):
        """The f16 start latents [n,4,h,w] of an img2img denoise (the img2img pipeline's add_noise): alpha*x0 + sigma_t*z at the first executed sigma
        of `schedule`.  x0_stride: elements between the x0 of two frames, 0 when one serves all; z as _draw_start returns it."""
        self.scheduler.set_timesteps(*schedule[:2])
        alpha, sigma_t = (float(np.float32(v)) for v in self.scheduler.add_noise_coefficients())
        same = self.cfg.noise_mode.lower() == "same"
        assert z.shape[0] == (1 if same else n)
        chw = 4 * z.shape[-2] * z.shape[-1]
        out = torch.empty(n, *z.shape[1:], dtype=H16, device=self.dev)
        self.L.tcl_light_start_f16(out, x0.contiguous(), x0_stride, z.contiguous(), 0 if same else chw, n, chw, alpha, sigma_t, stream())
        return out

    def _axis_ramp(self, side, H, W, levels=None):
        """One axis-aligned ramp in the [0,1] convention VAEEngine.encode takes, [1,3,H,W] f32 = uint8(linspace)/254.  side: the TCL_LIGHT_* index
        naming the axis; levels None: tcl_light_gradient_f32 (255 at that side, 0 opposite), else (first, last) sample of tcl_bg_ramp_f32."""
        img = torch.empty(1, 3, H, W, dtype=torch.float32, device=self.dev)
        if levels is None:
            self.L.tcl_light_gradient_f32(img, H, W, side, stream())
        else:
            self.L.tcl_bg_ramp_f32(img, H, W, side, int(levels[0]), int(levels[1]), stream())
        return img

    def bg_ramp(self, source, H, W):
        """bg_source left | right | top | bottom | grey: the ramp (or flat grey) of HL.BG_RAMPS."""
        side, start, stop = HL.BG_RAMPS[source]
        return self._axis_ramp(side, H, W, (start, stop))

    def matte_grey(self, frames, alpha, sigma=None):
        """The background demo's run_rmbg composite: frames [n,3,H,W] f32, alpha [n,1,H,W] f32 -> trunc(clamp(127 + (255 f - 127) a))/254.
        sigma (process_normal's run_rmbg(img, sigma=16)): 127 + ((255 f - 127) + sigma) a."""
        n, _, H, W = frames.shape
        out = torch.empty(n, 3, H, W, dtype=torch.float32, device=self.dev)
        if sigma is None:
            self.L.tcl_matte_grey_f32(frames.float().contiguous(), alpha.float().contiguous(), out, n, H, W, stream())
        else:
            self.L.tcl_matte_grey_sigma_f32(frames.float().contiguous(), alpha.float().contiguous(), out, n, H, W, float(sigma), stream())
        return out

    def foreground(self, frames, sigma=None):
        """The foreground image of the fbc model -> (fg_frames [n,3,H,W] f32, alpha [n,1,H,W] | None): the frames matted onto grey with BriaRMBG's
        alpha (matte_grey), or, with fbc_matting false, as they are (alpha None, no RMBGEngine needed)."""
        if not self.cfg.fbc_matting:
            return frames.float().contiguous(), None
        if self.rmbg is None:
            raise RuntimeError("generation.fbc_matting needs an RMBGEngine (Generator(..., rmbg=...)); fbc_matting: false feeds the frames as they are")
        alpha = self.rmbg.estimate_alpha(frames, self.batch_size)
        return self.matte_grey(frames, alpha, sigma), alpha

    def prepare_fbc(self, frames, background):
        """The two condition images of the fbc model: fg_frames [n_local,3,H,W] (matted onto grey, or as given) and bg_frames [1|n_local,3,H,W]
        (bg_source).  A background of one frame serves every frame and is encoded once."""
        c = self.cfg
        n, _, H, W = frames.shape
        self.fg_frames, self.fbc_alpha = self.foreground(frames)
        self.bg_index = None
        if self.light:                     # bg_frames = the DISTINCT ramps of this rank's frames; __call__ encodes those and gathers the latents
            self.bg_frames, index, several = self.light_images(n, H, W)
            if several:
                self.bg_index = torch.tensor(index, dtype=torch.long, device=self.dev)
        elif c.bg_source in HL.BG_RAMPS:
            self.bg_frames = self.bg_ramp(c.bg_source, H, W)
        else:
            if background is None or background.dim() != 4 or background.shape[0] not in (1, n) or tuple(background.shape[1:]) != (3, H, W):
                raise ValueError(f"generation.bg_source {c.bg_source}: background frames {None if background is None else tuple(background.shape)}, "
                                 f"expected {(1, 3, H, W)} or {(n, 3, H, W)}")
            bg = background.to(frames).float()
            self.bg_frames = (torch.flip(bg, dims=[-1]) if c.bg_source == "upload_flip" else bg).contiguous()

    # ------------------------------------------------------------------ normals (gradio_demo_bg_iclight.py: process_normal)
    def fbc_normal(self, left, right, bottom, top, alpha=None):
        """Four decoded relights [n,3,H,W] f32 and the matting alpha [n,1,H,W] f32 (None: 1 everywhere) -> (normal_u8 [n,H,W,3] u8 with
        RGB = (u, v, h), ambient [n,3,H,W] f32): one tcl_fbc_normal launch."""
        n, _, H, W = left.shape
        srcs = [t.float().contiguous() for t in (left, right, bottom, top)]
        if any(tuple(t.shape) != (n, 3, H, W) for t in srcs) or (alpha is not None and tuple(alpha.shape) != (n, 1, H, W)):
            raise ValueError(f"fbc_normal: relights {[tuple(t.shape) for t in srcs]}, alpha {None if alpha is None else tuple(alpha.shape)}; "
                             f"expected four of {(n, 3, H, W)} and {(n, 1, H, W)}")
        a = 0 if alpha is None else alpha.float().contiguous()
        normal = torch.empty(n, H, W, 3, dtype=torch.uint8, device=self.dev)
        ambient = torch.empty(n, 3, H, W, dtype=torch.float32, device=self.dev)
        self.L.tcl_fbc_normal(*srcs, a, normal, 0, ambient, n, H, W, stream())
        return normal, ambient

    @torch.no_grad()
    def normals(self, frames, conds, conds_t, n_total=None):
        """generation.normal: frames = this rank's block [n_local,3,H,W] f32 in [0,1]; conds / conds_t as in __call__.
        The matte (sigma = 16; fbc_matting false: the frames as they are, alpha = 1) and the foreground latents are made once.  Per direction of
        HL.NORMAL_SIDES: the ramp's single frame is encoded, the start is made again exactly as prepare_data makes it and VidToMe's generator is put
        back to where it stood at entry (the demo seeds a generator per process() call), then ddim_sample and the decode -- so each direction is, bit
        for bit, the plain run with that bg_source.  One tcl_fbc_normal launch over the block; multi-rank results are all-gathered.
        bg_source, stage 1 / 2 and the highres pass play no part.
        Returns (normal_u8 [N,H,W,3] u8, ambient [N,3,H,W] f32, {side: relit frames [N,3,H,W] f32}, info)."""
        c, d = self.cfg, self.dist
        if not self.normal_sides:
            raise ValueError("Generator.normals needs generation.normal: true (and generation.iclight_model fbc)")
        self._bg_per_frame = False          # every direction's ramp is one frame for all
        n, _, H, W = frames.shape
        self._total(n, n_total, keep=False)
        ev = self._now
        t0 = ev()
        self.fg_frames, alpha = self.foreground(frames, sigma=HL.NORMAL_MATTE_SIGMA)
        self.frames = frames.contiguous()
        fg = self.vae.encode_imgs_batch(self.fg_frames, self.batch_size)
        tome_rng = getattr(self.unet.tome, "rng", None)
        tome_state = None if tome_rng is None else tome_rng.bit_generator.state
        t1 = ev()
        relit, denoise, encode, decode = {}, {}, t1 - t0, 0.0
        for side in self.normal_sides:
            ta = ev()
            if tome_state is not None:
                tome_rng.bit_generator.state = tome_state
            self.bg_frames = self.bg_ramp(side, H, W)
            bg = self.vae.encode_imgs_batch(self.bg_frames, self.batch_size)
            self.prepare_start(n, H, W)
            tb = ev()
            x = self.ddim_sample(self.init_noise.clone(), conds, conds_t, (fg, bg))
            tc = ev()
            relit[side] = self.vae.decode_latents_batch(x, self.batch_size)
            denoise[side], encode, decode = tc - tb, encode + (tb - ta), decode + (ev() - tc)
        t2 = ev()
        normal, ambient = self.fbc_normal(*(relit[s] for s in HL.NORMAL_SIDES), alpha)
        if d.multi:
            normal, ambient = d.gather_frames(normal, self.n_total), d.gather_frames(ambient, self.n_total)
            relit = {s: d.gather_frames(r.contiguous(), self.n_total) for s, r in relit.items()}
        t3 = ev()
        self.timing = dict(encode=encode, denoise=sum(denoise.values()), decode=decode, normal=t3 - t2, total=t3 - t0)
        info = dict(timing=self.timing, denoise_per_direction=denoise, total_time=t3 - t0, sec_per_frame=(t3 - t0) / self.n_total,
                    total_number_of_frames=self.n_total, iclight_model=c.iclight_model, normal=True, apply_opt=False,
                    scheduler_steps=self.schedule[0], steps_executed=self.schedule[2],
                    max_memory_allocated=torch.cuda.max_memory_allocated(self.dev) / 1024.0 ** 2)
        return normal, ambient, relit, info

    def light_gradient(self, side, H, W):
        """The demo's bg_source image (gradio_demo_iclight.py:241-256) in VAEEngine.encode's [0,1] convention: [1,3,H,W] f32 = uint8(linspace)/254."""
        return self._axis_ramp(HL.INIT_LATENTS.index(side) - 1, H, W)

    def light_ramps(self, angles, H, W, hi, lo):
        """generation.light_path: the ramps of frames at `angles` (degrees).  Frames are grouped by bitwise-equal reduced angle and every distinct
        angle is rendered once, in [0,1] convention [1,3,H,W] f32 = u/254: an exact multiple of 90 takes the image of the existing kernels
        (tcl_light_gradient_f32 at the levels (255, 0), tcl_bg_ramp_f32 otherwise), so a constant path at 0 / 90 / 180 / 270 is the left / top / right /
        bottom run bit for bit; all the others leave in one tcl_light_ramp_angle_f32 launch.
        Returns (images [D,3,H,W] f32 in order of first appearance, [index into them per frame])."""
        reduced = [HL.light_reduce(a) for a in angles]
        distinct, index = [], []
        for r in reduced:                  # floats of [0, 360) without -0.0: equal values are equal bits
            if r not in distinct:
                distinct.append(r)
            index.append(distinct.index(r))
        general = [r for r in distinct if HL.light_axis_side(r) is None]
        swept = None
        if general:
            swept = torch.empty(len(general), 3, H, W, dtype=torch.float32, device=self.dev)
            dirs = torch.tensor(HL.light_dirs(general), dtype=torch.float64).to(self.dev)
            self.L.tcl_light_ramp_angle_f32(swept, dirs, len(general), H, W, int(hi), int(lo), stream())
            if len(general) == len(distinct):
                return swept, index
        images = []
        for r in distinct:
            side = HL.light_axis_side(r)
            if side is None:
                images.append(swept[general.index(r)][None])
            elif (hi, lo) == HL.LIGHT_LEVELS["fc"]:
                images.append(self.light_gradient(side, H, W))
            else:
                images.append(self._axis_ramp(HL.INIT_LATENTS.index(side) - 1, H, W, (hi, lo) if side in ("left", "top") else (lo, hi)))
        return (images[0] if len(images) == 1 else torch.cat(images)), index

    def light_images(self, n, H, W):
        """The ramps of this rank's n frames under generation.light_path, from the frames' GLOBAL positions (a rank of a sharded run builds what one
        rank would): (distinct images [D,3,H,W], [index per local frame], whether the run as a whole has more than one distinct ramp -- the same
        answer on every rank, as the per-frame background of fbc needs it)."""
        c = self.cfg
        n_total = self._total(n)
        lo, hi = self.dist.range(n_total)
        assert hi - lo == n
        angles = HL.light_angles(c.light_path, HL.light_positions(n_total))
        self.light_angles = angles[lo:hi]
        several = len({HL.light_reduce(a) for a in angles}) > 1
        images, index = self.light_ramps(self.light_angles, H, W, *HL.LIGHT_LEVELS[c.iclight_model])
        return images, index, several

    def frame_text(self, uncond, keys, n, n_total=None):
        """generation.prompt_path: the per-frame text of this rank's n frames, from the frames' GLOBAL positions (a rank of a sharded run builds the
        rows of the frames it denoises).  uncond [L,768] f16: the negative prompt; keys [P,L,768] f16: the distinct keyframe prompts in the order of
        HL.prompt_table (text.encode_prompt_set).  Frames with equal (k0, k1, t) share a row; all rows leave in one tcl_text_lerp_f16 launch, t rounded
        from f64 to f32 once.  -> unet.FrameText, which takes the place of `conds` in __call__ / ddim_sample."""
        c = self.cfg
        if c.prompt_path is None:
            raise ValueError("Generator.frame_text needs generation.prompt_path")
        n_total = self._total(n, n_total)
        lo, hi = self.dist.range(n_total)
        assert hi - lo == n
        prompts, rows, index = HL.prompt_table(c.prompt_path, n_total, lo, hi)
        keys = keys.to(self.dev).to(H16).contiguous()
        if keys.dim() != 3 or keys.shape[0] != len(prompts):
            raise ValueError(f"generation.prompt_path: {len(prompts)} distinct keyframe prompts, embeddings {tuple(keys.shape)}")
        h_tab = torch.tensor([[k0, k1, struct.unpack("<i", struct.pack("<f", t))[0]] for k0, k1, t in rows], dtype=I32)
        out = torch.empty(len(rows), *keys.shape[1:], dtype=H16, device=self.dev)
        self.L.tcl_text_lerp_f16(out, keys, len(prompts), h_tab.to(self.dev), h_tab, len(rows), keys.shape[1] * keys.shape[2], stream())
        self.prompt_rows = rows
        return FrameText(uncond.to(self.dev), out, index)

    def build_start(self, concat_conds):
        """img2img start (gradio_demo_iclight.py:283-299 -> the img2img pipeline's add_noise): init_noise = alpha*x0 + sigma_t*z at the first executed
        sigma, with z the f32 draw of prepare_data and x0 the light gradient's latent (encoded once, shared by all frames) or, for `source`,
        the frames' own clean latents `concat_conds` [n_local,4,h,w] f16, or, under light_path, the latent of each frame's own ramp."""
        c = self.cfg
        n, chw = self.frames.shape[0], 4 * self.h * self.w
        if c.init_latent == "source":
            x0, x0_stride = concat_conds.contiguous(), chw
            if tuple(x0.shape) != (n, 4, self.h, self.w) or x0.dtype != H16:
                raise ValueError(f"init_latent 'source': clean latents {tuple(x0.shape)} {x0.dtype}, expected {(n, 4, self.h, self.w)} f16")
        elif self.light:                   # the distinct ramps are encoded, in batches of batch_size, and gathered to the frames; one ramp serves all
            images, index, _ = self.light_images(n, *self.frames.shape[-2:])
            x0, x0_stride = self.vae.encode_imgs_batch(images, self.batch_size).contiguous(), 0
            if x0.shape[0] > 1:
                x0, x0_stride = x0[torch.tensor(index, dtype=torch.long, device=self.dev)].contiguous(), chw
        else:
            x0, x0_stride = self.vae.encode(self.light_gradient(c.init_latent, *self.frames.shape[-2:])).contiguous(), 0
        self.init_noise = self._noised_start(n, x0, x0_stride, self.start_noise, self.schedule)
        return self.init_noise

    # ------------------------------------------------------------------ highres pass (gradio_demo_iclight.py:301-334)
    def frames_to_u8(self, frames):
        """[n,3,H,W] f32 as decode_latents_batch returns it -> [n,H,W,3] u8, u = trunc(clamp(fl32(255 p), 0, 255)) (the demo's pytorch2numpy
        computes y * 127.5 + 127.5 on the [-1,1] image: the same value up to f32 rounding at integer boundaries)."""
        n, _, H, W = frames.shape
        out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=self.dev)
        self.L.tcl_frames_to_u8(frames.float().contiguous(), out, n, H, W, stream())
        return out

    def _lanczos_table(self, n_in, n_out):
        """The device table of one resampled axis (host f64, C library: csrc/resize.hip), made once per size pair; None for an unchanged axis."""
        if n_in == n_out:
            return None
        if (n_in, n_out) not in self._lanczos:
            ints = self.L.tcl_resize_lanczos_table_ints(n_in, n_out)
            if ints == 0:
                raise ValueError(f"LANCZOS resize {n_in} -> {n_out}: the ratio is outside [0.25, 2]")
            t = torch.empty(ints, dtype=I32)
            self.L.tcl_resize_lanczos_table(n_in, n_out, t)
            self._lanczos[(n_in, n_out)] = t.to(self.dev)
        return self._lanczos[(n_in, n_out)]

    def resize_lanczos_u8(self, u8, H2, W2):
        """[n,H,W,3] u8 -> [n,H2,W2,3] u8, PIL's Image.resize((W2, H2), Image.LANCZOS) of every frame, bit for bit."""
        n, H, W, _ = u8.shape
        tx, ty = self._lanczos_table(W, W2), self._lanczos_table(H, H2)
        out = torch.empty(n, H2, W2, 3, dtype=torch.uint8, device=self.dev)
        self.L.tcl_resize_lanczos_u8(u8.contiguous(), out, n, H, W, H2, W2, 0 if tx is None else tx, 0 if ty is None else ty, stream())
        return out

    def u8_to_frames(self, u8):
        """[n,H,W,3] u8 -> [n,3,H,W] f32 = u/254: VAEEngine.encode's 2x - 1 is then the demo's u/127 - 1 (numpy2pytorch), as in light_gradient."""
        n, H, W, _ = u8.shape
        out = torch.empty(n, 3, H, W, dtype=torch.float32, device=self.dev)
        self.L.tcl_u8_to_frames_f32(u8.contiguous(), out, n, H, W, 254.0, stream())
        return out

    def highres_upscale(self, decoded):
        """decoded [n,3,H,W] f32 (the first pass's frames) -> (u8 [n,H2,W2,3], x0 [n,4,H2/8,W2/8] f16): quantise, LANCZOS resize to
        HL.highres_size, back to float as u/254, VAE encode in batches of batch_size."""
        H2, W2 = HL.highres_size(*decoded.shape[-2:], self.cfg.highres_scale)
        up = self.resize_lanczos_u8(self.frames_to_u8(decoded), H2, W2)
        x0 = torch.cat([self.vae.encode(self.u8_to_frames(b)) for b in up.split(self.batch_size, dim=0)])
        return up, x0

    def highres_start(self, x0):
        """The second pass's start latents: alpha*x0 + sigma_t*z at the first executed sigma of schedule_highres, z a fresh f32 draw from rng_dev
        (noise_mode same: one frame for all; vanilla: n_total frames, this rank's block taken, as prepare_data does)."""
        n, _, h2, w2 = x0.shape
        return self._noised_start(n, x0, 4 * h2 * w2, self._draw_start(h2, w2), self.schedule_highres)

    def highres_pass(self, x, frames_hr, conds, conds_t):
        """x: the first pass's latents [n_local,4,h,w]; frames_hr: this rank's source frames at the final size [n_local,3,H2,W2] f32 in [0,1] (the
        project's own loader at that size, not the demo's LANCZOS crop).  -> the refined latents [n_local,4,H2/8,W2/8]; the Generator's working
        size is the final one from here on."""
        n = x.shape[0]
        H2, W2 = HL.highres_size(8 * self.h, 8 * self.w, self.cfg.highres_scale)
        if frames_hr is None or tuple(frames_hr.shape) != (n, 3, H2, W2):
            raise ValueError(f"highres pass: source frames at the final size {None if frames_hr is None else tuple(frames_hr.shape)}, "
                             f"expected {(n, 3, H2, W2)}")
        if getattr(self.unet.tome, "enabled", True):
            HL.check_highres_tokens(H2, W2, self.cfg.chunk_size)
        self.upscaled_u8, x0 = self.highres_upscale(self.vae.decode_latents_batch(x, self.batch_size))
        self.frames = frames_hr.float().contiguous()
        concat_conds = self.vae.encode_imgs_batch(self.frames, self.batch_size)
        start = self.highres_start(x0)
        self.h, self.w = H2 // 8, W2 // 8
        return self.ddim_sample(start, conds, conds_t, concat_conds, schedule=self.schedule_highres)

    def _load_start_latents(self, n):
        """generate.py:563-566, 191-194: start from the saved latents of the scheduler's first timestep when they exist (-> True); nothing is
        drawn from the RNG then, as in the reference.  The file covers the video, `frame_ids` picks this run's frames, the rank takes its block."""
        c = self.cfg
        # the file is named after the first timestep, so prepare_data sets the scheduler's timesteps here (generate.py:561 does it before prepare_data
        # too); ddim_sample sets them again, and set_timesteps depends on nothing but n_timesteps
        self.scheduler.set_timesteps(c.n_timesteps)
        t0 = self.scheduler.timesteps[0]
        path = get_latents_dir(c.latents_path, c.model_key)
        found = check_latent_exists(path, [t0])
        print(f"[INFO] latent path {f'found at {path}' if found else 'not found, generating new latents.'}")
        if not found:
            return False
        try:
            z = load_latent(path, t0, c.frame_ids)
        except IndexError as e:
            raise ValueError(f"start latents under {path} do not cover frame_ids: {e}") from e
        lo, hi = self.dist.range(self.n_total)
        if not torch.is_tensor(z) or tuple(z.shape) != (self.n_total, 4, self.h, self.w):
            raise ValueError(f"start latents under {path}: {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__} after the frame selection, "
                             f"expected {(self.n_total, 4, self.h, self.w)} = [frames, 4, H/8, W/8]")
        self.init_noise = z[lo:hi].to(self.dev).to(H16).contiguous()
        assert self.init_noise.shape[0] == n
        return True

    # ------------------------------------------------------------------ one UNet evaluation with CFG
    def _groups(self, chunks, tokens_per_frame):
        """Consecutive chunks per UNet pass: as many as fit `max_tokens_per_pass` (activation memory); order is preserved, so every
        block still meets the chunks in the reference order."""
        cap = max(1, int(self.cfg.max_tokens_per_pass) // (2 * tokens_per_frame))
        groups, cur, n = [], [], 0
        for c in chunks:
            if cur and n + len(c) > cap:
                groups.append(cur); cur, n = [], 0
            cur.append(c); n += len(c)
        if cur:
            groups.append(cur)
        return groups

    def _run_groups(self, groups, Hh, Ww, t, text, pack, unpack, ip=None):
        """One block-major UNet pass per group of chunks.  pack(grp) -> (xin, idx, n); unpack(eps, idx, n)."""
        for grp in groups:
            xin, idx, n = pack(grp)
            # per-frame text (prompt_path, xy passes only): the UNet needs to know which frame each sample is
            kw = dict(frames=[f for c in grp for f in c]) if isinstance(text, FrameText) else {}
            if ip is not None:             # generation.ip_adapter (xy passes only)
                kw["ip"] = ip
            eps = self.unet.forward_many(xin, [len(c) for c in grp], Hh, Ww, t, text, cfg_pair=True, **kw)     # the pack kernel wrote both halves
            unpack(eps, idx, n)

    def _unet_xy(self, x, cc, chunks, text, t, noises):
        """pred_noise on the xy chunks of one step (generate.py:220-224, 288-352): chunks = lists of local frame ids, reference order.
        The chunks go through the UNet in block-major passes (`forward_many`, see unet.py): one pack, one unpack per pass."""
        def pack(grp):
            return self._pack(x, cc, [f for c in grp for f in c], 0, 0, 0, self.h, self.w)

        def unpack(eps, idx, n):
            self.L.tcl_unpack_cfg_f16(eps, idx, n, 0, 0, 0, self.h, self.w, float(self.cfg.guidance_scale), 0, 1.0, 0, noises, stream())

        self._run_groups(self._groups(chunks, self.h * self.w), self.h, self.w, t, text, pack, unpack, ip=self.ip)

    def _unet_yt(self, x_full, cc_full, items, nt_full, text_t, t):
        """pred_noise on the yt chunks of one frame window: 'n c h w -> w c n h' (generate.py:265-273); items share (start, length)."""
        sl, nwin, _, scale_upto, nkeep = items[0]

        def pack(grp):
            return self._pack(x_full, cc_full, [c for ch in grp for c in ch], 1, sl, nwin, nwin, self.h)

        def unpack(eps, idx, n):
            self.L.tcl_unpack_cfg_f16(eps, idx, n, 1, sl, nwin, self.h, self.w, float(self.cfg.guidance_scale), scale_upto, math.sqrt(0.5),
                                      nkeep, nt_full, stream())

        self._run_groups(self._groups([it[2] for it in items], nwin * self.h), nwin, self.h, t, text_t, pack, unpack)

    def _pack(self, x, cc, ids, axis, start, window, rows, cols):
        """The UNet input of one pass, both CFG halves: [2 n, rows, cols, 8 | 12] f16 for the samples `ids` -- frames of x (axis 0) or latent columns of
        the frame window (start, window) (axis 1).  cc: the condition latents in the form ddim_sample takes them, a tensor (fc) or the pair
        (foreground, background [1 | frames]) (fbc, checked by _check_fbc_conds).  -> (xin, ids on the device, n)."""
        n = len(ids)
        idx = torch.tensor(ids, dtype=I32, device=self.dev)
        if isinstance(cc, (tuple, list)):
            fg, bg = cc
            xin = torch.empty(2 * n, rows, cols, 12, dtype=H16, device=self.dev)
            self.L.tcl_pack_latents12_f16(x, fg, bg, bg.shape[0], idx, n, axis, start, window, self.h, self.w, xin, stream())
        else:
            xin = torch.empty(2 * n, rows, cols, 8, dtype=H16, device=self.dev)
            self.L.tcl_pack_latents_f16(x, cc, idx, n, axis, start, window, self.h, self.w, xin, stream())
        return xin, idx, n

    def _yt_items(self, w_chunks):
        """(window start, length, columns, scale_upto, nkeep) in the reference's loop order (generate.py:265-278)."""
        starts, ovl = HL.temporal_windows(self.n_total, self.cfg.win_size_t)
        items = []
        for k, sl in enumerate(starts):
            nwin = min(self.cfg.win_size_t, self.n_total - sl)
            nkeep = (starts[k + 1] - sl) if k + 1 < len(starts) else nwin
            up = sl + ovl[k - 1] if k > 0 else 0
            for ch in w_chunks:
                items.append((sl, nwin, ch, up, nkeep))
        return items

    def _check_fbc_conds(self, x, concat_conds):
        """fbc: concat_conds is the pair (foreground [n_local,4,h,w], background [1|n_local,4,h,w]) of contiguous f16 latents -- the pack kernel
        reads them by frame index, so their extents are checked here, on the host, once per denoise."""
        n = x.shape[0]
        if not isinstance(concat_conds, (tuple, list)) or len(concat_conds) != 2:
            raise ValueError("iclight_model fbc: concat_conds is the pair (foreground latents, background latents)")
        fg, bg = concat_conds
        per_frame = bg.shape[0] > 1 if self._bg_per_frame is None else self._bg_per_frame      # the entry point's word, when it gave one
        ok_bg = bg.shape[0] == (n if per_frame else 1) and tuple(bg.shape[1:]) == (4, self.h, self.w)
        if tuple(fg.shape) != (n, 4, self.h, self.w) or not ok_bg or fg.dtype != H16 or bg.dtype != H16 or not (fg.is_contiguous() and bg.is_contiguous()):
            raise ValueError(f"iclight_model fbc: foreground latents {tuple(fg.shape)} {fg.dtype}, background latents {tuple(bg.shape)} {bg.dtype}; "
                             f"expected {(n, 4, self.h, self.w)} and {(n if per_frame else 1, 4, self.h, self.w)} contiguous f16")
        return per_frame

    def _conds_full(self, x, concat_conds):
        """Once per denoise: the fbc pair is checked, and for the yt passes (alpha_t > 0, else None) the conditions of ALL frames are gathered, in
        the form they came in -- the background of fbc only when it is one per frame."""
        d, yt = self.dist, self.cfg.alpha_t > 0
        if self.fbc:
            per_frame = self._check_fbc_conds(x, concat_conds)
            fg, bg = concat_conds
            return (d.gather_frames(fg, self.n_total), d.gather_frames(bg, self.n_total) if per_frame else bg) if yt else None
        return d.gather_frames(concat_conds, self.n_total) if yt else None

    # ------------------------------------------------------------------ hot loop 1
    @torch.no_grad()
    def ddim_sample(self, x, conds, conds_t, concat_conds, schedule=None):
        """schedule: (scheduler steps, begin index, steps executed) of an img2img entry other than the first pass's own (the highres pass)."""
        c, d = self.cfg, self.dist
        sch = self.scheduler
        if schedule is not None:
            sch.set_timesteps(*schedule[:2])
        elif self.img2img:     # enter the longer schedule at its begin index: sch.timesteps are the executed steps, so the decay `alphas` and the
            sch.set_timesteps(*self.schedule[:2])      # "no noise on the last step" rule below are taken over them, counted from 0
        else:
            sch.set_timesteps(c.n_timesteps)
        n_local = x.shape[0]
        noises = torch.zeros_like(x)
        noises_t = torch.zeros_like(x)
        alphas = HL.alpha_schedule(c.alpha_t, c.final_factor_t, len(sch.timesteps))
        xy_sampler = HL.ChunkSampler(c.seed + 7919 * d.rank, c.chunk_size, c.merge_global, c.chunk_ord)
        yt_sampler = HL.ChunkSampler(c.seed + 1, c.chunk_size, c.merge_global, c.chunk_ord)
        cc_full = self._conds_full(x, concat_conds)
        lo, hi = d.range(self.n_total)
        warp_steps = c.noise_warp is not None and c.noise_warp["steps"]      # the per-step noise is a chain over the flows too
        for i, t in enumerate(sch.timesteps.tolist()):
            self._unet_xy(x, concat_conds, xy_sampler.get_chunks(n_local), conds, t, noises)
            if c.alpha_t > 0:
                items = self._yt_items(yt_sampler.get_chunks(self.w))
                nt = sharded_temporal_pass(d, x, cc_full, self.n_total, items,
                                           lambda xf, cf, its, out: self._unet_yt(xf, cf, its, out, conds_t, t))
                noises_t.copy_(nt)
                self.L.tcl_adain_fuse_f16(noises_t, noises, n_local * 4, self.h * self.w, float(alphas[i]), stream())
            z = None
            if i < len(sch.timesteps) - 1:     # the last SDE step has sigma_t = 0: its noise term vanishes
                if warp_steps:
                    zf = self._warp_chain(self.h, self.w)
                else:
                    zf = torch.randn(self.n_total, 4, self.h, self.w, generator=self.rng_dev, device=self.dev, dtype=torch.float32)
                z = zf[lo:hi].to(H16).contiguous()
            sch.step(noises, t, x, noise=z)
            self.unet.tome.reset_global_tokens()       # post_iter (generate_utils.py:235-238)
        return x

    # ------------------------------------------------------------------ end to end
    def __call__(self, frames, conds, conds_t, past_flows, mask_bwds, unq_inv, n_total=None, k=None, background=None, frames_hr=None,
                 background_per_frame=None, source=None, flows=None, keyframes=None):
        """frames: local block [n_local,3,H,W]; conds / conds_t: [2,L,768] f16 (uncond, cond) text embeddings for the xy / yt
        passes (generate.py:553-555) -- under generation.prompt_path conds is the FrameText of frame_text; past_flows / mask_bwds / unq_inv: stage-2 inputs for ALL frames (device).
        With generation.noise_mode warp: past_flows / mask_bwds are needed whether stage 1 / 2 run or not -- the noise is carried along them.
        Returns (relit frames [N,3,H,W] f32, info dict).
        With generation.highres_scale > 1: frames_hr is the local block at HL.highres_size [n_local,3,H2,W2], the stage-2 inputs live at that size
        and so do the returned frames.
        With generation.iclight_model fbc: background [1|n_local,3,H,W] is the bg_source upload / upload_flip image (one frame for all, or this
        rank's block of a per-frame clip); background_per_frame says which when the block alone cannot (None: more than one frame handed in) --
        every rank must give the same answer, since a per-frame background is all-gathered for the yt pass.
        With generation.detail_transfer: source [N,3,H,W] f32 in [0,1] holds the source frames of ALL ranks at the size of the result (the final size
        under the highres pass); see detail_step.
        With generation.keyframes: frames (and a per-frame background) are this rank's block of the KEY frames only, n_total their number,
        keyframes=their frame numbers in the clip (HL.keyframe_ids), flows=(fut, past) [N,2,H,W] the flows between all consecutive frames of the clip
        and source all its N frames, both at the size of the result; the stage-2 inputs belong to all N frames, as do the returned frames; see
        propagate_step."""
        c, d = self.cfg, self.dist
        if self.highres and background is not None:
            raise ValueError("generation.background_cond together with generation.highres_scale > 1 is not supported")
        self._total(frames.shape[0], n_total, keep=False)
        if (c.prompt_path is not None) != isinstance(conds, FrameText) or (isinstance(conds, FrameText) and len(conds.index) != frames.shape[0]):
            raise ValueError("generation.prompt_path: conds must be the FrameText of Generator.frame_text for this rank's frames (and only then)")
        n_out = self.n_total                  # the frames returned: with generation.keyframes all frames of the clip, of which n_total are denoised
        keys = None
        if c.keyframes is not None:
            if keyframes is None:
                raise ValueError("generation.keyframes: the frame numbers of the key frames are missing (Generator(...)(..., keyframes=...))")
            keys = [int(k) for k in keyframes]
            n_out = keys[-1] + 1
            if len(keys) != self.n_total or HL.keyframe_ids(n_out, c.keyframes["interval"]) != keys:
                raise ValueError(f"generation.keyframes: keyframes {keys} are not the {self.n_total} key frames of a clip at interval "
                                 f"{c.keyframes['interval']} (hostlogic.keyframe_ids)")
            if source is None or source.dim() != 4 or source.shape[0] != n_out:
                raise ValueError(f"generation.keyframes: source frames {None if source is None else tuple(source.shape)}, expected all {n_out} "
                                 "frames of the clip at the size of the result (Generator(...)(..., source=...))")
            if flows is None or len(flows) != 2 or any(f is None or f.dim() != 4 or f.shape[0] != n_out for f in flows):
                raise ValueError(f"generation.keyframes: flows are missing or not (fut, past) over all {n_out} frames of the clip at the size of "
                                 "the result (Generator(...)(..., flows=...))")
        elif keyframes is not None and len(keyframes) != self.n_total:
            raise ValueError("generation.keyframes is off: keyframes= must be left out (or name every frame)")
        detail = c.detail_transfer is not None and c.detail_transfer["blend"] > 0.0      # blend 0: nothing runs, the frames are returned as they are
        if detail and (source is None or source.dim() != 4 or source.shape[0] != n_out):
            raise ValueError(f"generation.detail_transfer: source frames {None if source is None else tuple(source.shape)}, expected all "
                             f"{n_out} frames of the run at the size of the result (Generator(...)(..., source=...))")
        ev = self._now
        t0 = ev()
        self.prepare_data(frames, background, past_flows, mask_bwds)
        # fbc: is the background one frame per frame?  Under light_path when the run has several ramps, else the caller's word (None: by its length)
        self._bg_per_frame = (self.bg_index is not None) if self.light else (None if background_per_frame is None else bool(background_per_frame))
        concat_conds = self.encode_conds()
        if self.img2img:
            self.build_start(concat_conds)
        t1 = ev()
        x = self.ddim_sample(self.init_noise.clone(), conds, conds_t, concat_conds)
        self.latents = x                   # the first pass's result (with highres on: what the second pass starts from)
        t2 = t2a = ev()
        if self.highres:                   # decode -> u8 -> resize -> encode -> second denoise, between `denoise` and `decode`
            x = self.highres_pass(x, frames_hr, conds, conds_t)
            t2 = ev()
        mode = "shard" if c.shard_post_opt else str(c.post_opt_mode)
        if mode not in ("replicated", "replicated_all", "global", "shard"):
            raise ValueError(f"post_opt_mode {mode!r}: expected replicated | replicated_all | global | shard")
        shard = d.multi and mode == "shard" and c.apply_opt
        clean, past_flows, mask_bwds, unq_inv, k = self.decode_gather(x, shard, past_flows, mask_bwds, unq_inv, k)
        t3 = ev()
        holes = None
        if keys is not None:               # the frames between the keys, at the final size; stage 1 / 2 and detail_step see all frames of the clip
            clean, holes = self.propagate_step(clean, source, flows, keys)
        t3p = t4 = t5 = t3 if keys is None else ev()
        losses1 = losses2 = None
        if c.apply_opt:
            clean, losses1, losses2, t4 = self.post_optimize(clean, mode, shard, past_flows, mask_bwds, unq_inv, k)
            t5 = ev()
        t6 = t5
        if detail:
            clean = self.detail_step(clean, source)
            t6 = ev()
        self.timing = dict(encode=t1 - t0, denoise=t2a - t1, decode=t3 - t2, stage1=t4 - t3p, stage2=t5 - t4, total=t6 - t0)
        info = dict(timing=self.timing, losses_exposure=losses1, losses_unique=losses2, total_time=t6 - t0,
                    sec_per_frame=(t6 - t0) / n_out, total_number_of_frames=n_out, init_latent=c.init_latent,
                    iclight_model=c.iclight_model, ip_adapter=c.ip_adapter,
                    init_strength=c.init_strength, scheduler_steps=self.schedule[0], steps_executed=self.schedule[2],
                    max_memory_allocated=torch.cuda.max_memory_allocated(self.dev) / 1024.0 ** 2)
        if keys is not None:
            self.timing["propagate"] = t3p - t3
            between = (n_out - len(keys)) * clean.shape[-2] * clean.shape[-1]
            info["keyframes"] = dict(interval=c.keyframes["interval"], denoised=len(keys), holes=int(holes.sum().item()) / between if between else 0.0)
        if detail:
            self.timing["detail"] = t6 - t5
            info["detail"] = dict(c.detail_transfer)
        if self.highres:
            self.timing["highres"] = t2 - t2a
            info.update(highres_scale=c.highres_scale, highres_denoise=c.highres_denoise, highres_size=[8 * self.h, 8 * self.w],
                        highres_scheduler_steps=self.schedule_highres[0], highres_steps_executed=self.schedule_highres[2])
        return clean, info

    def propagate_step(self, clean, source, flows, keys):
        """generation.keyframes: clean [M,3,H,W], the decoded key frames of all ranks -> ([N,3,H,W] all frames of the clip, holes [N]): the keys bit
        for bit, every frame in between its source frame times the gain field relit / source of its two neighbouring keys, carried along the chained
        flows and blended by distance (keyframe.propagate).  It runs at the final size, behind the decode and the highres pass, where the flows and
        the source frames live, and in front of stage 1 / 2, which smooth the whole clip along its tracks.  Every rank does the whole clip, no
        collective."""
        from .keyframe import propagate
        b = self.cfg.keyframes
        fut, past = (f.float().contiguous() for f in flows)
        return propagate(source.float().contiguous(), clean.float().contiguous(), keys, fut, past, b["alpha"], b["diff_threshold"], b["eps"])

    def detail_step(self, clean, source):
        """generation.detail_transfer, the last step: clean [N,3,H,W], the frames __call__ is about to return (all of the run's, on every rank) ->
        the same with the high frequencies of `source`, which must match them frame for frame.  It runs behind stage 1 / 2: stage 2's codebook
        averages along tracks and would smooth re-injected detail, and both stages stay what they are without the key.  Every rank does the whole
        clip, no collective.  Under fbc the weight is the matting alpha: on one rank the one prepare_fbc estimated, with several ranks it is
        estimated again on the full source (a rank holds the alpha of its own block only)."""
        from .detail import detail_transfer
        c = self.cfg
        if source is None or tuple(source.shape) != tuple(clean.shape):
            raise ValueError(f"generation.detail_transfer: source frames {None if source is None else tuple(source.shape)}, expected "
                             f"{tuple(clean.shape)} -- all frames of the run at the size of the result (Generator(...)(..., source=...))")
        mask = None
        if self.fbc:
            mask = self.fbc_alpha
            if mask is None or mask.shape[0] != clean.shape[0]:
                mask = self.rmbg.estimate_alpha(source, self.batch_size)
            mask = mask.float().contiguous()
        b = c.detail_transfer
        return detail_transfer(source.float().contiguous(), clean.float().contiguous(), b["sigma"], b["mode"], b["blend"], b["channels"], mask)

    def encode_conds(self):
        """ddim_sample's concat_conds from what prepare_data left.  fc: the latents of the frames.  fbc: the pair (foreground, background) latents
        (model_utils.py:97-179 concat_conds, kept apart: one background frame stays one); under light_path bg_frames are the distinct ramps and
        their latents are gathered to one per frame."""
        enc = lambda images: self.vae.encode_imgs_batch(images, self.batch_size)
        if self.fbc:
            fg, bg = enc(self.fg_frames), enc(self.bg_frames)
            return fg, (bg if self.bg_index is None else bg[self.bg_index].contiguous())
        return enc(self.frames)

    def decode_gather(self, x, shard, past_flows, mask_bwds, unq_inv, k):
        """The latents of this rank's frames -> (decoded frames, then the stage-1 / 2 inputs that go with them).  Multi-rank: the frames of all ranks,
        decoded slab by slab, every slab in an async all-gather while the next one decodes (parallel.gather_frames_pipelined).
        shard (opt-in approximation): the rank keeps its own block as a video of its own -- its first frame has no predecessor, tracks are cut at
        the block boundary; the global track ids restricted to the block and renumbered densely give the partition get_flowid would produce when
        started at the block's first frame.  No collective, but NOT the reference's result."""
        d = self.dist
        if d.multi and not shard:
            clean = d.gather_frames_pipelined(lambda a, b: self.vae.decode_latents_batch(x[a:b], self.batch_size), x.shape[0], self.n_total,
                                              slab=int(os.environ.get("TCL_DECODE_SLAB", "8")))
            return clean, past_flows, mask_bwds, unq_inv, k
        clean = self.vae.decode_latents_batch(x, self.batch_size)
        if shard:
            lo, hi = d.range(self.n_total)
            past_flows, mask_bwds = past_flows[lo:hi], mask_bwds[lo:hi]
            hw = clean.shape[-2] * clean.shape[-1]
            uniq, inv_local = torch.unique(unq_inv[lo * hw:hi * hw], return_inverse=True)
            unq_inv, k = inv_local.to(torch.int32), int(uniq.numel())
        return clean, past_flows, mask_bwds, unq_inv, k

    def post_optimize(self, clean, mode, shard, past_flows, mask_bwds, unq_inv, k):
        """Stage 1 (exposure alignment) and stage 2 (unique video tensor) on the decoded frames under post_opt_mode `mode` (DEFAULTS).
        -> (frames, stage-1 losses, stage-2 losses | None, the timing point between the stages)."""
        c, d = self.cfg, self.dist
        N = clean.shape[0]
        pd = d if (mode == "global" and d.multi) else None      # global: the ranks split every mini-batch and share one parameter set;
        #                                                           # replicated / shard: every rank optimises on its own (no collective)
        pd1 = d if (mode in ("global", "replicated") and d.multi) else None      # stage 1: dealt over the ranks unless replicated_all / shard
        ds = post_opt.OptDataset(clean, past_flows, mask_bwds, device=self.dev)
        rng = np.random.default_rng(c.seed + (d.rank if shard else 0))      # global mode: the identical schedule on every rank
        s1 = post_opt.make_schedule(N, c.batch_size, c.epochs_exposure, rng)
        _, _, losses1 = post_opt.exposure_align(ds, s1, c.epochs_exposure, c.batch_size, c.exposure_lr_init, c.exposure_lr_final,
                                                c.lambda_dssim, c.lambda_flow, dist=pd1)
        t4 = self._now()
        losses2 = None
        if c.epochs > 0:
            s2 = post_opt.make_schedule(N, c.batch_size, c.epochs, rng)
            clean, _, losses2 = post_opt.unique_tensor_optimization(ds, unq_inv, s2, c.batch_size, c.feature_lr, c.lambda_dssim,
                                                                    c.lambda_flow, c.lambda_tv, k=k, dist=pd)
        else:
            clean = ds.edited_images
        if shard:
            clean = d.gather_frames(clean.contiguous(), self.n_total)
        return clean, losses1, losses2, t4
