"""What a generation.normal run costs beside one fbc relight: seeded random weights at the SD-1.5 / AutoencoderKL sizes, a synthetic clip at 1280x720,
fbc_matting off (no RMBG engine), apply_opt off.  One plain fbc run (bg_source left) warms the allocator and the GEMM table, a second one is timed,
then Generator.normals on the same frames.  Prints one JSON line.   python tools/micro/normal_run.py [--json out.json] [--frames N] [--steps K]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tc_light_amd import sd15  # noqa: E402
from tc_light_amd.generate import Generator  # noqa: E402
from tc_light_amd.unet import UNetEngine  # noqa: E402
from tc_light_amd.vae import VAEEngine  # noqa: E402
from tc_light_amd.vidtome import VidToMe  # noqa: E402

H, W = 720, 1280


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    n, steps = arg("--frames", 24), arg("--steps", 20)
    unet = UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(in_channels=12), seed=1), "cuda", VidToMe("cuda", seed=5))
    vae = VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")
    g = torch.Generator().manual_seed(0)
    frames = torch.rand(n, 3, H, W, generator=g).cuda()
    conds = torch.randn(2, 77, 768, generator=g).half().cuda()
    cfg = dict(n_timesteps=steps, alpha_t=0.01, seed=31, apply_opt=False, iclight_model="fbc", fbc_matting=False)
    res = dict(frames=n, size=[H, W], steps=steps, alpha_t=0.01)
    for tag in ("warm", "fbc_left"):
        unet.tome = VidToMe("cuda", seed=5)
        _, info = Generator(unet, vae, dict(cfg, bg_source="left"))(frames, conds, conds, None, None, None)
        res[tag] = {k: round(float(v), 3) for k, v in info["timing"].items()}
    unet.tome = VidToMe("cuda", seed=5)
    _, _, _, info = Generator(unet, vae, dict(cfg, normal=True)).normals(frames, conds, conds)
    res["normals"] = {k: round(float(v), 3) for k, v in info["timing"].items()}
    res["normals"]["denoise_per_direction"] = {s: round(float(t), 3) for s, t in info["denoise_per_direction"].items()}
    res["normals"]["sec_per_frame"] = round(info["sec_per_frame"], 4)
    line = json.dumps(res)
    print(line)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
