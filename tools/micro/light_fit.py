"""Time tcl_light_fit_u8 (csrc/lightfit.hip, the sums behind evaluate.py --light) at 60 frames of 1280x720 against the plain torch composition of the
same ten sums on the same device (f32 luma, the clipping mask, the log ratio, ten masked reductions in f64).

Inputs: random uint8 clips E and S [N,3,H,W] on the device.  Both are warmed up, then timed alternately (`--repeats` rounds of `--calls` calls, host
clock around a device synchronise).  Bytes moved = what the algorithm has to read once, 6 B per pixel; GB/s = that over the median time, so the
torch figure is an equivalent rate, not its traffic.  The two results are compared (relative difference per sum) and reported, not asserted.
    python tools/micro/light_fit.py [--frames 60 --height 720 --width 1280] [--once]    (--once: one call of the kernel, for a profiler)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def torch_sums(E, S):
    """The same ten sums with torch primitives: E, S uint8 [N,3,H,W] -> f64 [N,10]."""
    N, _, H, W = E.shape

    def luma(x):
        x = x.float()
        return ((0.299 * x[:, 0] + 0.587 * x[:, 1]) + 0.114 * x[:, 2]) / 255.0
    ye, ys = luma(E), luma(S)
    lo, hi = 2.0 / 255.0, 253.0 / 255.0
    w = ((ye >= lo) & (ye <= hi) & (ys >= lo) & (ys <= hi)).float()
    r = torch.log((ye + 1.0 / 255.0) / (ys + 1.0 / 255.0)) * w
    u = ((2.0 * torch.arange(W, device=E.device) + 1.0) / W - 1.0).view(1, 1, W) * w
    v = ((2.0 * torch.arange(H, device=E.device) + 1.0) / H - 1.0).view(1, H, 1) * w
    terms = (w, u, v, u * u, u * v, v * v, r, r * u, r * v, r * r)
    return torch.stack([t.sum(dim=(1, 2), dtype=torch.float64) for t in terms], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "light_fit needs a GPU"
    dev = torch.device("cuda:0")
    from tc_light_amd.lib import lib, stream
    n, h, w = a.frames, a.height, a.width
    g = torch.Generator(device=dev).manual_seed(3)
    E = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device=dev, generator=g)
    S = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device=dev, generator=g)
    L = lib()
    ws = torch.empty(L.tcl_light_fit_workspace_bytes(n, h, w) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(n, 10, dtype=torch.float64, device=dev)            # the workspace and the output are allocated once, outside the timed window
    hip = lambda: L.tcl_light_fit_u8(E, S, n, h, w, out, ws, stream())
    if a.once:
        hip(); torch.cuda.synchronize()
        hip(); torch.cuda.synchronize()
        print(json.dumps({"sums_frame0": out[0].tolist()}))
        return
    ref = lambda: torch_sums(E, S)
    hip(); got_t = ref(); hip(); ref(); torch.cuda.synchronize()
    got_h = out.clone()
    rel = ((got_h - got_t).abs() / got_t.abs().clamp(min=1.0)).max(dim=0).values.tolist()
    times = {"hip": [], "torch": []}
    for _ in range(a.repeats):
        for name, f in (("hip", hip), ("torch", ref)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.calls * 1e3)
    M = n * h * w
    nbytes = 6 * M
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"shape": {"frames": n, "height": h, "width": w}, "pixels": M, "bytes_algorithm": nbytes,
           "hip_ms": times["hip"], "torch_ms": times["torch"], "hip_ms_median": med["hip"], "torch_ms_median": med["torch"],
           "hip_GBps": nbytes / (med["hip"] * 1e-3) / 1e9, "torch_GBps_equivalent": nbytes / (med["torch"] * 1e-3) / 1e9,
           "torch_over_hip": med["torch"] / med["hip"], "max_rel_diff_per_sum": rel,
           "how": f"{a.repeats} alternating rounds of {a.calls} calls after warm-up, host clock around a device synchronise"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
