"""The u8 leg of the highres pass at the default size: tcl_frames_to_u8, tcl_resize_lanczos_u8 (1280x720 -> 1920x1088) and tcl_u8_to_frames_f32 on 8 frames
per launch, device events around the calls after a warm-up at the same shapes.  Bytes moved are what the algorithm needs (input read once, output
written once), computed from the shapes.  Prints one JSON line.   python tools/micro/highres_resize.py [--json out.json] [--frames N] [--reps R]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tc_light_amd import hostlogic as HL  # noqa: E402
from tc_light_amd.lib import lib, stream  # noqa: E402

H, W, SCALE = 720, 1280, 1.5


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
    n, reps = arg("--frames", 8), arg("--reps", 200)
    L = lib()
    H2, W2 = HL.highres_size(H, W, SCALE)
    g = torch.Generator().manual_seed(0)
    frames = torch.rand(n, 3, H, W, generator=g).cuda()
    u8 = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda")
    up = torch.empty(n, H2, W2, 3, dtype=torch.uint8, device="cuda")
    img = torch.empty(n, 3, H2, W2, device="cuda")
    tabs = []
    for a, b in ((W, W2), (H, H2)):
        t = torch.empty(L.tcl_resize_lanczos_table_ints(a, b), dtype=torch.int32)
        L.tcl_resize_lanczos_table(a, b, t)
        tabs.append(t.cuda())
    res = dict(frames=n, size_in=[H, W], size_out=[H2, W2], reps=reps)
    for name, fn, nbytes in (
            ("frames_to_u8", lambda: L.tcl_frames_to_u8(frames, u8, n, H, W, stream()), n * H * W * 3 * (4 + 1)),
            ("resize_lanczos_u8", lambda: L.tcl_resize_lanczos_u8(u8, up, n, H, W, H2, W2, tabs[0], tabs[1], stream()), n * 3 * (H * W + H2 * W2)),
            ("u8_to_frames_f32", lambda: L.tcl_u8_to_frames_f32(up, img, n, H2, W2, 254.0, stream()), n * H2 * W2 * 3 * (1 + 4))):
        t = events(fn, reps)
        res[name] = dict(us_per_launch=t * 1e6, us_per_frame=t / n * 1e6, bytes=nbytes, gbs=nbytes / t / 1e9)
    line = json.dumps(res)
    print(line)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
