"""The cost of generation.noise_mode warp at the default size (1280x720), 60 frames, multi-axis denoising on, 10 steps, apply_opt off: the Generator run
(seeded random weights, the same frames) under one noise_mode per process, after a warm-up.  The flows are synthetic -- a camera that pans by
(3, 1) pixels and zooms by 1.02 per frame, masks 1 -- so the chain meets copies, stretched sources and fresh strips as a moving ego camera gives them.
    python tools/micro/noise_warp_cost.py --mode vanilla|same|warp [--frames N] [--steps S] [--rounds K] [--root DIR] [--json out.json]
With --root DIR the package is imported from another checkout (the parent commit): the form of the same-box comparison, one process per tree,
alternating.  --mode warp also times the chain alone (tcl_noise_warp_count + tcl_noise_warp_apply_f32 + the draws, 60 frames, device events) and
reports its rate against the modelled bytes: per pixel 36 B cleared, 28 B read and 36 B of atomics in count, 48 B read and 16 B written in apply."""
import json
import os
import statistics
import sys


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


sys.path.insert(0, os.path.abspath(arg("--root", os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), str)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 720, 1280
BYTES_PER_PIXEL = 36 + 28 + 36 + 48 + 16


def camera_flows(n, dev):
    """Backward flows [n,2,H,W] of a pan by (3, 1) and a zoom by 1.02 about the centre per frame, masks [n,1,H,W] = 1."""
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    u = (x - (W - 1) / 2) / 1.02 - (x - (W - 1) / 2) - 3.0
    v = (y - (H - 1) / 2) / 1.02 - (y - (H - 1) / 2) - 1.0
    f = torch.stack([u, v]).float()[None].repeat(n, 1, 1, 1)
    f[0] = 0
    return f.contiguous(), torch.ones(n, 1, H, W, device=dev)


def main():
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    from tc_light_amd import sd15
    from tc_light_amd.generate import Generator
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vae import VAEEngine
    from tc_light_amd.vidtome import VidToMe
    n, steps, rounds, mode = arg("--frames", 60), arg("--steps", 10), arg("--rounds", 2), arg("--mode", "vanilla", str)
    dev = torch.device("cuda")
    unet = UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(), seed=1), dev, VidToMe(dev, seed=12345))
    vae = VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), dev)
    g = np.random.default_rng(5)
    frames = torch.rand(n, 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    emb = torch.from_numpy(g.standard_normal((4, 77, 768)).astype(np.float32)).to(dev).half()
    conds, conds_t = emb[:2].contiguous(), emb[[0, 3]].contiguous()
    base = dict(alpha_t=0.01, final_factor_t=0.01, seed=12345, apply_opt=False, noise_mode=mode)
    past, masks = camera_flows(n, dev) if mode == "warp" else (None, None)

    def run(n_steps):
        unet.tome = VidToMe(dev, seed=12345)                         # the same coins for every run
        gen = Generator(unet, vae, dict(base, n_timesteps=n_steps, frame_ids=list(range(n))))
        _, info = gen(frames, conds, conds_t, past, masks, None, n_total=n)
        return info

    run(2)                                                           # warm-up
    runs = []
    for _ in range(rounds):
        info = run(steps)
        runs.append(dict(total=info["total_time"], **{k: float(v) for k, v in info["timing"].items() if k != "total"}))
    res = dict(mode=mode, frames=n, size=[H, W], steps=steps, rounds=rounds, device=torch.cuda.get_device_name(0),
               total_seconds=dict(median=statistics.median(r["total"] for r in runs), all=[r["total"] for r in runs]), runs=runs)
    if mode == "warp":
        from tc_light_amd.noisewarp import field_draw, warp_chain
        rng = torch.Generator(device=dev).manual_seed(1)
        draw = field_draw(rng, dev)
        held = [draw(H, W) for _ in range(4)]                        # the chain without its draws: fields drawn before the clock starts
        count = [0]

        def replay(h, w):
            count[0] += 1
            return held[count[0] % 4]
        times = {}
        for name, d in (("chain_with_draws", draw), ("chain_kernels_only", replay)):
            warp_chain(d, past, masks, n, H, W)
            ms = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                warp_chain(d, past, masks, n, H, W)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            times[name] = dict(ms_median=statistics.median(ms), ms_all=ms)
        gb = BYTES_PER_PIXEL * H * W * (n - 1) / 1e9
        k = times["chain_kernels_only"]["ms_median"]
        res["chain"] = dict(times, modelled_gb=gb, gb_per_s=gb / (k / 1e3), chains_per_run=steps, seconds_per_run=steps * times["chain_with_draws"]["ms_median"] / 1e3)
    line = json.dumps(res)
    print(line)
    if "--json" in sys.argv:
        out = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
