"""The cost of generation.prompt_path at the default size (1280x720), 60 frames, multi-axis denoising on.
A two-keyframe path over N frames has N distinct text rows: every conditional sample of an xy pass attends to K / V panels of its own, where the
single-prompt run reads one pair of panels for the whole guidance half.  This script runs the same denoise (seeded random weights, the same frames,
apply_opt off) both ways, alternating, after a warm-up of both, and reports the `denoise` phase of each run, the bytes the per-frame K / V panels
hold, and the peak memory of either mode.
    python tools/micro/prompt_path_cost.py [--frames N] [--steps S] [--rounds K] [--only single|path] [--json out.json]
--only runs one mode alone (one warm-up, one timed denoise): the form to put under `rocprofv3 --kernel-trace --stats`, where the attention of the
per-frame text is the kernel k_flash_kvi and everything else that attends is k_flash."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 720, 1280
A, B = "sunrise, soft pink light low on the left", "dusk, warm orange light low on the right"


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    from tc_light_amd import hostlogic as HL, sd15
    from tc_light_amd.generate import Generator
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vae import VAEEngine
    from tc_light_amd.vidtome import VidToMe
    n, steps, rounds, only = arg("--frames", 60), arg("--steps", 10), arg("--rounds", 2), arg("--only", None, str)
    dev = torch.device("cuda")
    unet = UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(), seed=1), dev, VidToMe(dev, seed=12345))
    vae = VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), dev)
    g = np.random.default_rng(5)
    frames = torch.rand(n, 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    emb = torch.from_numpy(g.standard_normal((4, 77, 768)).astype(np.float32)).to(dev).half()      # negative, A, B; the yt pair below
    conds_t = emb[[0, 3]].contiguous()
    base = dict(alpha_t=0.01, final_factor_t=0.01, seed=12345, apply_opt=False, frame_ids=list(range(n)))
    path = HL.prompt_sweep(A, B)
    assert len(HL.prompt_table(path, n)[1]) == n                    # all rows distinct

    def run(mode, n_steps):
        cfg = dict(base, n_timesteps=n_steps, **(dict(prompt_path=path) if mode == "path" else {}))
        gen = Generator(unet, vae, cfg)
        conds = gen.frame_text(emb[0], emb[1:3].contiguous(), n, n_total=n) if mode == "path" else emb[:2].contiguous()
        torch.cuda.reset_peak_memory_stats(dev)
        _, info = gen(frames, conds, conds_t, None, None, None, n_total=n)
        return info["timing"]["denoise"], torch.cuda.max_memory_allocated(dev), gen.cfg.max_tokens_per_pass

    modes = [only] if only else ["single", "path"]
    for m in modes:
        run(m, 2)                                                   # warm-up: every shape's tile, the text K / V of both kinds of text
    secs, peak, tokens = {m: [] for m in modes}, {}, {}
    for _ in range(1 if only else rounds):
        for m in modes:
            t, p, tok = run(m, steps)
            secs[m].append(t)
            peak[m], tokens[m] = p, tok
    res = dict(frames=n, size=[H, W], steps=steps, rows=n, text_tokens=77,
               denoise_seconds={m: dict(median=statistics.median(v), all=v) for m, v in secs.items()},
               peak_bytes=peak, max_tokens_per_pass=tokens,
               kv_panel_bytes_single=unet.text_rows_bytes(2), kv_panel_bytes_path=unet.text_rows_bytes(1 + n),
               kv_projection_bytes_path=sum((1 + n) * 77 * 2 * blk["c"] * 2 for blk in unet.tfm.values()))
    if not only:
        a, b = res["denoise_seconds"]["single"]["median"], res["denoise_seconds"]["path"]["median"]
        res["path_over_single"] = b / a
    line = json.dumps(res)
    print(line)
    if "--json" in sys.argv:
        out = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
