"""DDIM inversion loop on the engine (tc_light_amd/invert.py): seconds per step and the share of the two inversion kernels.

  python tools/micro/invert_bench.py [--frames 60] [--height 720] [--width 1280] [--steps 25] [--batch 0 8]

Seeded random weights, random latents (the VAE is not part of the loop).  Per --batch value (inversion.batch_size; 0: one group as large as
max_tokens_per_pass allows) a two-step warm-up (GEMM shapes the tile table lacks are timed on first use), then the timed run.  The pack / step kernels
are bracketed with events on the launch stream; the GEMM share comes from the library's own launch timing (tcl_prof_begin / tcl_prof_end, class 0).
"""
import argparse
import ctypes
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from tc_light_amd import sd15
from tc_light_amd.config_utils import _wrap
from tc_light_amd.invert import Inverter
from tc_light_amd.lib import lib
from tc_light_amd.scheduler import DPMSolverSDEScheduler
from tc_light_amd.unet import UNetEngine
from tc_light_amd.vidtome import VidToMe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--batch", type=int, nargs="+", default=[0, 8])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    h, w = a.height // 8, a.width // 8
    eng = UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(), seed=1), dev, VidToMe(dev, seed=5))
    g = torch.Generator(device=dev).manual_seed(1)
    lat = torch.randn(a.frames, 4, h, w, generator=g, device=dev).half()
    cnd = torch.randn(1, 77, 768, generator=g, device=dev).half()
    text = torch.cat([cnd, cnd]).contiguous()
    L = lib()
    for bs in a.batch:
        def cfg(steps):
            return _wrap(dict(sd_version="iclight", model_key="iclight", seed=3, data=dict(scene_type="video", rgb_path=None, height=a.height, width=a.width),
                              inversion=dict(prompt="", steps=steps, save_steps=steps, batch_size=bs, control="none"), generation=dict(n_timesteps=steps)))
        warm = Inverter(SimpleNamespace(unet=eng, vae=None), DPMSolverSDEScheduler(), cfg(2))
        warm.ddim_inversion(lat, lat, text)
        inv = Inverter(SimpleNamespace(unet=eng, vae=None), DPMSolverSDEScheduler(), cfg(a.steps))
        marks = []

        def bracket(fn):
            def run(*args):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); out = fn(*args); e1.record()
                marks.append((e0, e1))
                return out
            return run
        inv._pack, inv._step = bracket(inv._pack), bracket(inv._step)
        n_steps = len(inv.timesteps())
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(dev)
        L.tcl_prof_begin(1)
        t0 = time.perf_counter()
        x = inv.ddim_inversion(lat, lat, text)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ms, fl, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
        L.tcl_prof_end(0, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(cnt))
        kern = sum(e0.elapsed_time(e1) for e0, e1 in marks) / 1e3
        inv.h, inv.w = h, w
        groups = [f for _, f, _ in inv._groups(a.frames)]
        print(f"invert {a.frames} frames {a.width}x{a.height}, {n_steps} distinct timesteps of {a.steps}, batch_size {bs or 'open'}: groups of {groups[0]} slots x {len(groups)}; "
              f"{dt:.2f} s, {dt / n_steps:.3f} s/step, {1e3 * dt / n_steps / a.frames:.2f} ms/frame/step; pack+step kernels {kern * 1e3:.2f} ms in {len(marks)} launches = "
              f"{100 * kern / dt:.3f} % of the loop; GEMM {ms.value / 1e3:.2f} s = {100 * ms.value / 1e3 / dt:.1f} %; peak memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.1f} GiB; "
              f"finite {bool(torch.isfinite(x).all())}", flush=True)


if __name__ == "__main__":
    main()
