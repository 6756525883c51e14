"""The cost of generation.light_path at the default size (1280x720), 60 frames.
  * tcl_light_ramp_angle_f32, 60 distinct angles in one launch (12*N*H*W = 663.6 MB written, nothing read but 60 pairs; several times the 256 MiB
    Infinity Cache, so the rate is an HBM write rate), 16 B path and scalar path, against this box's own write rate: a device fill of the same
    buffer (torch's fill kernel).  Device events after a warm-up, the two measured in alternating rounds; the median round is reported, with
    the spread.
  * Generator.build_start (seeded VAE weights, a stand-in UNet that is never run): a 60-frame sweep with 60 distinct angles (60 ramps rendered,
    encoded in batches of batch_size and gathered) against `init_latent: left` (one gradient, one encode), alternating, host clock around a device
    synchronise.  The difference is what the sweep adds to a run's `encode` phase.
Prints one JSON line.   python tools/micro/light_sweep.py [--json out.json] [--frames N] [--reps R] [--rounds K] [--no-vae]"""
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tc_light_amd import hostlogic as HL  # noqa: E402
from tc_light_amd.lib import lib, stream  # noqa: E402

H, W = 720, 1280


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n


def alternate(fns, reps, rounds):
    """{name: [seconds per call, one per round]}: every round times each candidate once, in turn, after a warm-up of all of them."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(events(fn, reps))
    return out


def main():
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    n, reps, rounds = arg("--frames", 60), arg("--reps", 200), arg("--rounds", 5)
    L = lib()
    angles = HL.light_angles([[0.0, 1.0], [1.0, 359.0]], HL.light_positions(n))          # n distinct angles, none axis-aligned
    assert len({HL.light_reduce(a) for a in angles}) == n and all(HL.light_axis_side(HL.light_reduce(a)) is None for a in angles)
    dirs = torch.tensor(HL.light_dirs(angles), dtype=torch.float64).cuda()
    buf = torch.empty(n * 3 * H * W + 4, device="cuda")
    out, off = buf[:n * 3 * H * W], buf[1:1 + n * 3 * H * W]                              # off: 4 B past a 16 B boundary -> the scalar path
    nbytes = 12 * n * H * W
    t = alternate(dict(ramp_angle=lambda: L.tcl_light_ramp_angle_f32(out, dirs, n, H, W, 255, 0, stream()),
                       fill=lambda: out.fill_(0.5),
                       ramp_angle_scalar_path=lambda: L.tcl_light_ramp_angle_f32(off, dirs, n, H, W, 255, 0, stream())), reps, rounds)
    res = dict(frames=n, size=[H, W], reps=reps, rounds=rounds, bytes=nbytes)
    for k, v in t.items():
        m = statistics.median(v)
        res[k] = dict(us_per_launch=m * 1e6, us_per_frame=m / n * 1e6, gbs=nbytes / m / 1e9, gbs_min=nbytes / max(v) / 1e9, gbs_max=nbytes / min(v) / 1e9)
    res["ramp_angle_share_of_fill"] = res["ramp_angle"]["gbs"] / res["fill"]["gbs"]
    if "--no-vae" not in sys.argv:
        from tc_light_amd import sd15
        from tc_light_amd.generate import Generator
        from tc_light_amd.vae import VAEEngine
        vae = VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")
        stub = SimpleNamespace(dev=torch.device("cuda"), tome=SimpleNamespace(args={}))
        frames = torch.zeros(n, 3, H, W, device="cuda")
        gens = {}
        for name, keys in (("sweep", dict(light_path=[[0.0, 1.0], [1.0, 359.0]])), ("left", dict(init_latent="left"))):
            g = Generator(stub, vae, dict(keys, init_strength=0.9, n_timesteps=25, seed=1, max_tokens_per_pass=1 << 20))
            g.prepare_data(frames)
            gens[name] = g

        def timed(g):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.build_start(None)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        for g in gens.values():
            timed(g)                                                                      # warm-up: every shape of both
        secs = {k: [] for k in gens}
        for _ in range(3):
            for k, g in gens.items():
                secs[k].append(timed(g))
        res["build_start_seconds"] = {k: dict(median=statistics.median(v), all=v) for k, v in secs.items()}
        res["sweep_extra_seconds"] = res["build_start_seconds"]["sweep"]["median"] - res["build_start_seconds"]["left"]["median"]
        res["sweep_extra_ms_per_frame"] = res["sweep_extra_seconds"] / n * 1e3
    line = json.dumps(res)
    print(line)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
