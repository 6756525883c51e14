"""DDIM inversion on the IC-Light UNet -- the producer of `generation.latents_path` (reference: invert.py:22-332, `Inverter`).

The reference's Inverter drives a 4-channel UNet and knows nothing of IC-Light's `concat_conds`; this one is that loop on the engine:

  frames -> vae.encode_imgs_batch -> clean latents x AND the IC-Light condition concat_conds (THE SOURCE FRAMES CONDITION THEIR OWN INVERSION: the
  UNet's channels 4-7 see, at every noise level, the clean latents of the frame whose noise is being recovered -- exactly what Generator feeds them
  when it later denoises from these latents) -> for t ascending: eps = unet([x | cc], t, text); x <- pred_next_x(x, eps)  (invert.py:151-173, 215-244)
  -> `<save_path>/<model_key>/noisy_latents_<t>.pt`, the file `Generator.prepare_data` reads (generate.py:563-566).

Differences from the reference's loop, all deliberate:
  * the master latents are f32 [N,4,h,w] on the device for the whole loop and only the UNet's input is f16: inversion integrates K steps, and rounding x
    to f16 at each of them is an error the generator's start noise never sees (the reference's autocast keeps x in whatever pred_next_x returns);
  * there is no classifier-free guidance, so the two "halves" of `forward_many`'s pair batch are both the same condition: text = [cond, cond], the first
    half of a group's frames sits in the "uncond" slots and the second half in the "cond" slots -- no slot is wasted (an odd group repeats its last
    frame in the spare slot and the duplicate is dropped).  Rows are independent because VidToMe is off: the reference's inverter never applies the
    patch, so the UNet runs with a `VidToMe(enabled=False)` of the inverter's own, swapped in for the duration of a pass;
  * the timesteps are the generation scheduler's (`DPMSolverSDEScheduler.set_timesteps(inversion.steps)`), reversed, consecutive duplicates dropped
    (Karras rounding repeats small timesteps; a repeated timestep is the identity); `final_alpha_cumprod = alphas_cumprod[0]` (SD-1.5:
    `set_alpha_to_one: false`);
  * one launch between two UNet passes: tcl_ddim_step_f32 updates the f32 planes and writes f16(x) into the persistent UNet input of the group.
One process only (frames are independent; sharding them over ranks is not built).
"""
import datetime
import math
import os

import numpy as np
import torch

from .config_utils import save_config
from .dataparser import VideoDataParser, get_latents_dir, latent_file, save_frames
from .generate import default_max_tokens_per_pass
from .hostlogic import check_fbc
from .lib import lib, stream
from .vidtome import VidToMe

H16 = torch.float16
I32 = torch.int32

SKIP_MESSAGE = "[INFO] sd_version 'iclight': no inversion needed, latents start from noise (reference run.py:13-22)"


def check_config(config):
    """Everything this inverter refuses, checked before a model is loaded or a frame is read."""
    if config.sd_version != "iclight":
        raise NotImplementedError("DDIM inversion for sd_version 2.1/2.0/1.5/depth is outside tc_light_amd's scope (SURVEY 2.1 #20): "
                                  "tc_light_amd implements the IC-Light path (sd_version: iclight)")
    inv = config.inversion
    if str(inv.get("control", "none")).lower() != "none":
        raise NotImplementedError(f"inversion.control '{inv.get('control')}': ControlNet-guided inversion is not built in tc_light_amd (control: none is)")
    if inv.get("use_blip"):
        raise NotImplementedError("inversion.use_blip: BLIP captioning is not built in tc_light_amd -- give inversion.prompt")
    scene_type = str(config.data.get("scene_type", "video")).lower()
    if scene_type in ("carla", "interiornet"):
        raise NotImplementedError(f"data.scene_type '{scene_type}': this dataparser is not yet built in tc_light_amd (video and sceneflow are)")
    if scene_type not in ("video", "sceneflow"):
        raise NotImplementedError(f"Scene type '{scene_type}' is not supported.")
    gen = config.get("generation") or {}          # the background-conditioned model is not inverted (hostlogic.check_fbc names it)
    check_fbc(gen.get("iclight_model"), gen.get("bg_source"), inversion=True)
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        raise NotImplementedError(f"WORLD_SIZE={world}: DDIM inversion runs in one process (frames are independent; sharding them over ranks is "
                                  "not built) -- run invert.py without torchrun")
    return scene_type


def inversion_timesteps(scheduler, steps):
    """`reversed(scheduler.timesteps)` (invert.py:153) without consecutive duplicates: strictly increasing, ending at timesteps[0]."""
    scheduler.set_timesteps(steps)
    ts = [int(t) for t in reversed(scheduler.timesteps.tolist())]
    return [t for i, t in enumerate(ts) if i == 0 or t != ts[i - 1]]


def ddim_coeffs(alphas_cumprod, timesteps):
    """timesteps ascending -> [(mu, sigma, mu_prev, sigma_prev)] in f64, one per level (invert.py:220-235): level i's `prev` is level i-1, and
    final_alpha_cumprod = alphas_cumprod[0] below the first.  Inversion steps TO level i with its tuple, sampling steps FROM level i with the same one."""
    out = []
    for i, t in enumerate(timesteps):
        a_t = float(alphas_cumprod[t])
        a_p = float(alphas_cumprod[timesteps[i - 1]]) if i > 0 else float(alphas_cumprod[0])
        out.append((math.sqrt(a_t), math.sqrt(1.0 - a_t), math.sqrt(a_p), math.sqrt(1.0 - a_p)))
    return out


class Inverter:
    def __init__(self, pipe, scheduler, config, lora=None):
        """pipe / scheduler: what `init_iclight` returns; lora: the lora.LoRASet the pipe was loaded with (its text-encoder part goes into the prompt
        embedding).  `Inverter(None, None, config)` is the entry point a caller transliterated from the reference's run.py holds: for iclight it says
        that no inversion is needed and returns."""
        self.config, self.pipe, self.scheduler, self.lora = config, pipe, scheduler, lora
        if pipe is None:
            return
        scene_type = check_config(config)
        inv = config.inversion
        self.unet, self.vae = pipe.unet, pipe.vae
        self.dev = self.unet.dev
        self.model_key = config.get("model_key")
        self.tome = VidToMe(self.dev, seed=int(config.get("seed", 123)), enabled=False)      # the inverter's own: never the generator's instance
        self.L = lib()
        self.prompt, self.recon, self.force = inv.prompt, bool(inv.get("recon")), bool(inv.get("force"))
        self.save_latents, self.steps, self.n_frames = bool(inv.get("save_intermediate")), int(inv.steps), inv.get("n_frames")
        self.batch_size = int(inv.get("batch_size") or 0)
        scheduler.set_timesteps(int(inv.get("save_steps") or inv.steps))
        self.timesteps_to_save = [int(t) for t in scheduler.timesteps.tolist()]
        scheduler.set_timesteps(self.steps)
        self.max_tokens_per_pass = inv.get("max_tokens_per_pass") or default_max_tokens_per_pass(self.unet, self.dev)
        config.max_memory_allocated, config.total_time = 0, 0
        if scene_type == "sceneflow":
            from .sceneflow import SceneFlowDataParser
            self.data_parser = SceneFlowDataParser(config.data, self.dev)
        else:
            self.data_parser = VideoDataParser(config.data, self.dev)
        config.input_path = self.data_parser.rgb_path

    # ------------------------------------------------------------------ schedule
    def timesteps(self):
        return inversion_timesteps(self.scheduler, self.steps)

    def generation_first_timestep(self):
        """The name the consumer will look for: `set_timesteps(generation.n_timesteps).timesteps[0]` (Generator._load_start_latents)."""
        n = int((self.config.get("generation") or {}).get("n_timesteps", self.steps))
        self.scheduler.set_timesteps(n)
        t0 = int(self.scheduler.timesteps[0])
        self.scheduler.set_timesteps(self.steps)
        return t0, n

    def check_latent_exists(self, save_path):
        """invert.py:260-269: the final latents and, with save_intermediate, every timestep of `save_steps`."""
        ts = [self.timesteps()[-1]] + (self.timesteps_to_save if self.save_latents else [])
        return all(os.path.exists(latent_file(save_path, t)) for t in ts)

    # ------------------------------------------------------------------ groups of the pair batch
    def _groups(self, n):
        """Consecutive frames per UNet pass, sized by `max_tokens_per_pass` like Generator._groups (every frame is ONE sample here: the physical slots of
        a group, 2 * ceil(frames / 2), stay under the cap); inversion.batch_size is only an upper bound.  -> [(idx int32 [F], F, F_valid)]."""
        slots = max(2, int(self.max_tokens_per_pass) // (self.h * self.w))
        cap = slots - slots % 2
        if self.batch_size > 0:
            cap = min(cap, self.batch_size)
        out = []
        for lo in range(0, n, cap):
            fr = list(range(lo, min(lo + cap, n)))
            hf = (len(fr) + 1) // 2
            phys = fr + [fr[-1]] * (2 * hf - len(fr))           # first half -> "uncond" slots, second half (+ the odd duplicate) -> "cond" slots
            out.append((torch.tensor(phys, dtype=I32, device=self.dev), 2 * hf, len(fr)))
        return out

    # ------------------------------------------------------------------ the three device operations of the loop
    def _pack(self, x, cond, idx, F):
        xin = torch.empty(F, self.h, self.w, 8, dtype=H16, device=self.dev)
        self.L.tcl_invert_pack_f16(x, cond, idx, x.shape[0], F, self.h, self.w, xin, stream())
        return xin

    def _eps(self, xin, F, t, text):
        return self.unet.forward_many(xin, [F // 2], self.h, self.w, t, text)

    def _step(self, x, eps, idx, F, F_valid, co, inversion, xin):
        self.L.tcl_ddim_step_f32(x, eps, idx, x.shape[0], F, F_valid, self.h, self.w, *(float(np.float32(c)) for c in co), int(inversion), xin, stream())

    def _run(self, x, cond, text, order, inversion, on_level=None):
        """x: f32 master [N,4,h,w] (updated in place); order: the levels to visit, as indices into the ascending timesteps."""
        ts = self.timesteps()
        coeffs = ddim_coeffs(self.scheduler.alphas_cumprod, ts)
        self.h, self.w = x.shape[-2:]
        groups = self._groups(x.shape[0])
        xins = [self._pack(x, cond, idx, F) for idx, F, _ in groups]
        prev, self.unet.tome = self.unet.tome, self.tome
        try:
            for i in order:
                for (idx, F, Fv), xin in zip(groups, xins):
                    eps = self._eps(xin, F, ts[i], text)
                    self._step(x, eps, idx, F, Fv, coeffs[i], inversion, xin)
                if on_level is not None:
                    on_level(ts[i], x)
        finally:
            self.unet.tome = prev
        return x

    @torch.no_grad()
    def ddim_inversion(self, latents, cond, text, save_path=None):
        """invert.py:151-173: clean latents [N,4,h,w] -> f32 latents at timesteps[0] (eps at the level being stepped TO).  cond: concat_conds f16."""
        print("[INFO] start DDIM Inversion!")
        x = latents.to(self.dev).float().contiguous()
        keep = set(self.timesteps_to_save) if (self.save_latents and save_path) else ()

        def on_level(t, xx):
            if t in keep:
                torch.save(xx.to(H16).cpu(), latent_file(save_path, t))
        ts = self.timesteps()
        self._run(x, cond, text, range(len(ts)), True, on_level)
        if save_path:
            pth = latent_file(save_path, ts[-1])
            torch.save(x.to(H16).cpu(), pth)
            print(f"[INFO] inverted latent saved to: {pth}")
        return x

    @torch.no_grad()
    def ddim_sample(self, x, cond, text):
        """invert.py:175-190: deterministic DDIM sampling back down the same timesteps (the other branch of pred_next_x)."""
        print("[INFO] reconstructing frames...")
        x = x.to(self.dev).float().clone().contiguous()
        return self._run(x, cond, text, range(len(self.timesteps()) - 1, -1, -1), False)

    def prepare_cond(self, prompt):
        """`inversion.prompt` through encode_prompt_pair(prompt, prompt): [2, L, 768], both halves the same condition (no guidance)."""
        from .model_utils import allow_random
        from .text import encode_prompt_pair
        models = self.config.get("models") or {}
        return encode_prompt_pair(prompt, prompt, self.dev, models.get("text_encoder"), allow_random=allow_random(models), lora=self.lora)

    # ------------------------------------------------------------------ invert.py:272-323
    @torch.no_grad()
    def __call__(self, save_path, frame_ids=None):
        cfg = self.config
        if self.pipe is None:
            if cfg.sd_version == "iclight":
                print(SKIP_MESSAGE)
                return
            check_config(cfg)
        t_last = self.timesteps()[-1]
        t_gen, n_gen = self.generation_first_timestep()
        if t_gen != t_last:
            raise ValueError(f"inversion.steps={self.steps} ends at timestep {t_last}, but generation.n_timesteps={n_gen} starts at {t_gen}: the "
                             f"generator would look for noisy_latents_{t_gen}.pt and ignore noisy_latents_{t_last}.pt")
        save_path = get_latents_dir(save_path, self.model_key)
        os.makedirs(save_path, exist_ok=True)
        if self.check_latent_exists(save_path) and not self.force:
            print(f"[INFO] inverted latents exist at: {save_path}. Skip inversion! Set 'inversion.force: True' to invert again.")
            return
        frames = self.data_parser.load_video(frame_ids)
        ids = list(range(len(frames)))
        if self.n_frames is not None:
            ids = ids[:int(self.n_frames)]
        frames = frames[ids].contiguous()
        cuda = self.dev.type == "cuda"
        if cuda:
            torch.cuda.reset_peak_memory_stats(self.dev)
        start = datetime.datetime.now()
        text = self.prepare_cond(self.prompt)
        with open(os.path.join(save_path, "inversion_prompts.txt"), "w") as f:
            f.write("\n".join([self.prompt] * len(frames)))
        latents = self.vae.encode_imgs_batch(frames, 2)          # clean latents AND concat_conds
        print(f"[INFO] clean latents shape: {tuple(latents.shape)}")
        x = self.ddim_inversion(latents, latents, text, save_path)
        save_config(cfg, save_path, inv=True)
        if cuda:
            torch.cuda.synchronize(self.dev)
            cfg.max_memory_allocated = torch.cuda.max_memory_allocated(self.dev) / 1024.0 ** 2
        cfg.total_time = (datetime.datetime.now() - start).total_seconds()
        if self.recon:
            rec = self.vae.decode_latents_batch(self.ddim_sample(x, latents, text).to(H16), 2)
            save_frames(rec, os.path.join(save_path, "recon_frames"), frame_ids=ids)
            mse = float(((rec.float().clamp(0, 1) - frames.float()) ** 2).mean())
            print(f"[INFO] reconstruction PSNR vs the source frames: {10.0 * math.log10(1.0 / max(mse, 1e-12)):.2f} dB over {len(ids)} frames")
        return x
