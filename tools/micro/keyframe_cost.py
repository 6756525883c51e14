"""The gain of generation.keyframes at the default size (1280x720), 60 frames, multi-axis denoising on, 10 steps, apply_opt off: the same Generator run
(seeded random weights, the same frames) at keyframes null, 2, 4 and 8, alternating in one process after a warm-up of every mode.  Reported per mode:
the run's total seconds (encode + denoise + decode + propagate), its phases, and the ratio to the plain run; beside them the seconds RAFT (seeded
stand-in weights) takes for the flows of the clip, which a keyframe run needs even when stage 1 / 2 are off -- `total_with_flows` adds them.
    python tools/micro/keyframe_cost.py [--frames N] [--steps S] [--rounds K] [--only null] [--root DIR] [--json out.json]
--only null runs the plain mode alone and touches nothing the key added; with --root DIR the package is imported from another checkout (the parent
commit): the form for the comparison of `keyframes: null` against the commit before, one process per tree, alternating."""
import json
import os
import statistics
import sys
import time


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


sys.path.insert(0, os.path.abspath(arg("--root", os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), str)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 720, 1280


def main():
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    from tc_light_amd import sd15
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
    emb = torch.from_numpy(g.standard_normal((4, 77, 768)).astype(np.float32)).to(dev).half()
    conds, conds_t = emb[:2].contiguous(), emb[[0, 3]].contiguous()
    base = dict(alpha_t=0.01, final_factor_t=0.01, seed=12345, apply_opt=False)
    modes = ["null"] if only == "null" else ["null", 2, 4, 8]
    flows, flow_seconds = None, None
    if only != "null":
        import warnings
        from tc_light_amd import hostlogic as HL
        from tc_light_amd.model_utils import load_raft_state
        from tc_light_amd.raft import RAFTEngine, estimate_flows_raft
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            raft = RAFTEngine(load_raft_state(None, allow=True), dev)
        estimate_flows_raft(raft, frames[:3])                        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flows = estimate_flows_raft(raft, frames)
        torch.cuda.synchronize()
        flow_seconds = time.perf_counter() - t0
        flows = tuple(f.float().contiguous() for f in flows)
        del raft

    def run(mode, n_steps):
        unet.tome = VidToMe(dev, seed=12345)                         # the same coins for every run
        if mode == "null":
            gen = Generator(unet, vae, dict(base, n_timesteps=n_steps, frame_ids=list(range(n))))
            _, info = gen(frames, conds, conds_t, None, None, None, n_total=n)
        else:
            keys = HL.keyframe_ids(n, mode)
            gen = Generator(unet, vae, dict(base, n_timesteps=n_steps, frame_ids=keys, keyframes=mode))
            _, info = gen(frames[keys].contiguous(), conds, conds_t, None, None, None, n_total=len(keys), source=frames, flows=flows, keyframes=keys)
        return info

    for m in modes:
        run(m, 2)                                                    # warm-up: every mode's shapes
    runs = {str(m): [] for m in modes}
    for _ in range(rounds):
        for m in modes:
            info = run(m, steps)
            runs[str(m)].append(dict(total=info["total_time"], **{k: float(v) for k, v in info["timing"].items() if k != "total"},
                                     **({k: info["keyframes"][k] for k in ("denoised", "holes")} if "keyframes" in info else {})))
    res = dict(frames=n, size=[H, W], steps=steps, rounds=rounds, flow_seconds=flow_seconds, device=torch.cuda.get_device_name(0),
               total_seconds={m: dict(median=statistics.median(r["total"] for r in v), all=[r["total"] for r in v]) for m, v in runs.items()}, runs=runs)
    if only != "null":
        plain = res["total_seconds"]["null"]["median"]
        res["total_over_plain"] = {m: v["median"] / plain for m, v in res["total_seconds"].items()}
        res["total_with_flows_over_plain"] = {m: (v["median"] + (0.0 if m == "null" else flow_seconds)) / plain for m, v in res["total_seconds"].items()}
        assert res["total_seconds"]["4"]["median"] < plain, "keyframes: 4 took no less total time than the plain run"
    line = json.dumps(res)
    print(line)
    if "--json" in sys.argv:
        out = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
