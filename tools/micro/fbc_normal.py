"""tcl_fbc_normal and tcl_matte_grey_sigma_f32 at the default size (1280x720), 16 frames per launch: device events around the calls after a warm-up
at the same shapes.  Bytes moved are what the algorithm needs (every input read once, every output written once), computed from the shapes; one
launch moves 1.2 GB, several times the 256 MiB Infinity Cache, so the rate is an HBM rate.  Prints one JSON line.
python tools/micro/fbc_normal.py [--json out.json] [--frames N] [--reps R]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tc_light_amd.lib import lib, stream  # noqa: E402

H, W = 720, 1280


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def events(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n


def main():
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    n, reps = arg("--frames", 16), arg("--reps", 50)
    L = lib()
    g = torch.Generator().manual_seed(0)
    base = torch.rand(n, 3, H, W, generator=g)
    rel = [(base + 0.3 * torch.rand(n, 3, H, W, generator=g) - 0.15).cuda() for _ in range(4)]
    alpha = torch.rand(n, 1, H, W, generator=g).cuda()
    frames = base.cuda()
    u8 = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda")
    f32 = torch.empty(n, 3, H, W, device="cuda")
    amb = torch.empty(n, 3, H, W, device="cuda")
    px = n * H * W
    res = dict(frames=n, size=[H, W], reps=reps)
    for name, fn, nbytes in (
            ("fbc_normal_all_outputs", lambda: L.tcl_fbc_normal(*rel, alpha, u8, f32, amb, n, H, W, stream()), px * (52 + 27)),
            ("fbc_normal_u8_ambient", lambda: L.tcl_fbc_normal(*rel, alpha, u8, 0, amb, n, H, W, stream()), px * (52 + 15)),
            ("fbc_normal_scalar_path", lambda: L.tcl_fbc_normal(*rel, alpha, u8.view(-1)[1:], 0, 0, n - 1, H, W, stream()),
             (n - 1) * H * W * (52 + 3)),
            ("matte_grey_sigma", lambda: L.tcl_matte_grey_sigma_f32(frames, alpha, f32, n, H, W, 16.0, stream()), px * (12 + 4 + 12))):
        t = events(fn, reps)
        res[name] = dict(us_per_launch=t * 1e6, us_per_frame=t / (n - 1 if "scalar" in name else n) * 1e6, bytes=nbytes, gbs=nbytes / t / 1e9)
    line = json.dumps(res)
    print(line)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
