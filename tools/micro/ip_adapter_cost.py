"""What generation.ip_adapter costs: tcl_attention_ip_add_f16 alone, the composition it replaces, and a multi-axis denoise with and without it.

  python tools/micro/ip_adapter_cost.py [--frames 60] [--height 720] [--width 1280] [--steps 25] [--reps 10] [--skip_denoise]

1. The kernel alone at the three level shapes of an xy pass over all frames (B = 2 x frames samples; C = 320 / 640 / 1280 at 1, 1/2, 1/4 of the latent
   size), Tip = 4: microseconds and GB/s over its 6 B per element of [M, C], beside a device copy that moves the same bytes (3 B per element read, 3
   written).
2. The composition it replaces at the same shapes: a second flash-attention launch over the 4 image keys (tcl_attention_f16, packing included, as
   attn2 would issue it) and an add pass a += scale * o (torch's, a stand-in for the pass one would write).
3. A multi-axis denoise (seeded random weights, random latents, no VAE) of --frames frames for --steps steps: without the adapter, with it, and without
   it but with attn2's fused query-panel route switched off (TCL_QPANEL=0) -- the route the adapter gives up at C = 320, so its share of the
   difference can be read off.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from tc_light_amd import ip_adapter as IP
from tc_light_amd import sd15
from tc_light_amd.generate import Generator
from tc_light_amd.lib import lib, stream
from tc_light_amd.unet import Ops, UNetEngine
from tc_light_amd.vidtome import VidToMe

H16 = torch.float16


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps           # microseconds


def kernel_legs(a, dev):
    L, ops = lib(), Ops(dev)
    B, Hd, Tip, scale = 2 * a.frames, sd15.HEADS, 4, 0.6
    h, w = a.height // 8, a.width // 8
    print(f"# kernel alone, Tip = {Tip}, B = {B} samples; bytes = 6 B x M x C")
    print(f"{'level':>5} {'N':>6} {'C':>5} {'M':>9} {'ip_add us':>10} {'GB/s':>7} {'copy us':>9} {'GB/s':>7} {'flash us':>9} {'add us':>8} {'flash+add us':>13}")
    for lvl, C in enumerate((320, 640, 1280)):
        N, d = h * w, C // Hd
        M = B * N
        g = torch.Generator(device=dev).manual_seed(lvl)
        q = torch.randn(M, C, device=dev, generator=g).half()
        att = torch.randn(M, C, device=dev, generator=g).half()
        kv = torch.randn(2, Tip, 2 * C, device=dev, generator=g).half()
        t_ip = timed(lambda: L.tcl_attention_ip_add_f16(q, C, N * C, kv, att, C, N * C, B, Hd, N, Tip, d, d ** -0.5, scale, B // 2, stream()), a.reps)
        nbytes = 6.0 * M * C
        src = torch.empty(3 * M * C, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t_cp = timed(lambda: dst.copy_(src), a.reps)
        del src, dst
        try:
            t_fl = timed(lambda: ops.attention(q, C, N * C, kv, 2 * C, Tip * 2 * C, kv[:, :, C:], 2 * C, Tip * 2 * C, B, Hd, N, Tip, d, kv_div=B // 2), a.reps)
            o2 = ops.attention(q, C, N * C, kv, 2 * C, Tip * 2 * C, kv[:, :, C:], 2 * C, Tip * 2 * C, B, Hd, N, Tip, d, kv_div=B // 2)
            t_add = timed(lambda: att.add_(o2, alpha=scale), a.reps)
            comp = f"{t_fl:9.1f} {t_add:8.1f} {t_fl + t_add:13.1f}"
        except RuntimeError as e:
            comp = f"(flash over {Tip} keys refused: {e})"
        print(f"{lvl:>5} {N:>6} {C:>5} {M:>9} {t_ip:10.1f} {nbytes / t_ip / 1e3:7.0f} {t_cp:9.1f} {nbytes / t_cp / 1e3:7.0f} {comp}")
        del q, att
        h, w = (h + 1) // 2, (w + 1) // 2


def denoise_legs(a, dev):
    tome = VidToMe(dev, seed=5)
    eng = UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(), seed=1), dev, tome)
    _, weights = IP.check_state(IP.seeded_state_dict(3))
    tokens = torch.randn(2, 4, 768, generator=torch.Generator().manual_seed(17)).half()
    ip = IP.make_prompt(tokens, weights, 0.6, dev)
    n, h, w = a.frames, a.height // 8, a.width // 8
    g = torch.Generator(device=dev).manual_seed(2)
    conds, conds_t = torch.randn(2, 77, 768, device=dev, generator=g).half(), torch.randn(2, 77, 768, device=dev, generator=g).half()
    cc = torch.randn(n, 4, h, w, device=dev, generator=g).half()
    state = tome.rng.bit_generator.state
    block = dict(image="reference", scale=0.6, path=None)

    def run(steps, prompt, env=None):
        os.environ.update(env or {})
        try:
            tome.rng.bit_generator.state = state
            tome.reset_global_tokens()
            gen = Generator(eng, None, dict(n_timesteps=steps, alpha_t=0.01, seed=7, ip_adapter=block if prompt is not None else None), image_prompt=prompt)
            gen.prepare_data(torch.zeros(n, 3, a.height, a.width, device=dev))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gen.ddim_sample(gen.init_noise.clone(), conds, conds_t, cc)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        finally:
            for k in env or {}:
                del os.environ[k]
    for prompt, env in ((None, None), (ip, None), (None, {"TCL_QPANEL": "0"})):       # warm-up: shapes the GEMM tile table lacks are timed on first use
        run(1, prompt, env)
    t_off, t_on, t_route = run(a.steps, None), run(a.steps, ip), run(a.steps, None, {"TCL_QPANEL": "0"})
    print(f"# multi-axis denoise, {n} frames {a.width}x{a.height}, {a.steps} steps (alpha_t 0.01), seconds")
    print(f"without the adapter                         {t_off:8.2f}")
    print(f"with the adapter (scale 0.6)                {t_on:8.2f}   (+{t_on - t_off:.2f} s, {100 * (t_on / t_off - 1):.1f} %)")
    print(f"without, query-panel route off (TCL_QPANEL=0) {t_route:6.2f}   (+{t_route - t_off:.2f} s: the un-fused route's share of the difference "
          f"{100 * (t_route - t_off) / max(t_on - t_off, 1e-9):.0f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip_denoise", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    kernel_legs(a, dev)
    if not a.skip_denoise:
        denoise_legs(a, dev)


if __name__ == "__main__":
    main()
