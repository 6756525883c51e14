"""Micro-benchmark of generation.detail_transfer: 60 frames of 1280x720, sigma 3 and sigma 16, both modes (channels rgb, no mask), the HIP call against the
same maths as a plain torch composition (two depthwise conv2d on reflect-padded input plus the element-wise operations) on the same box in the same run.

Every variant is warmed up, then the variants take turns for ROUNDS rounds; a round times REPS back-to-back calls between device events.  Reported per
variant: the median round's time per call, the spread (min .. max over the rounds), and GB/s over the bytes the algorithm must touch -- S and R read
once, O written once, 36 B per pixel.  The outputs of the two sides are compared on the timed inputs.

  python tools/micro/detail_bench.py [--frames 60] [--out profiles/detail_60x1280x720.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tc_light_amd import detail                                 # noqa: E402

ROUNDS, REPS = 7, 5


def torch_blur(x, taps):
    r = (taps.numel() - 1) // 2
    C = x.shape[1]
    x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (r, r, 0, 0), mode="reflect"), taps.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)
    return torch.nn.functional.conv2d(torch.nn.functional.pad(x, (0, 0, r, r), mode="reflect"), taps.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)


def torch_detail(S, R, taps, mode, blend):
    if mode == "add":
        D = S - R
        return (R + blend * (D - torch_blur(D, taps))).clamp_(0, 1)
    T = S * (torch_blur(R, taps) + 1.0 / 255.0) / (torch_blur(S, taps) + 1.0 / 255.0)
    return (R + blend * (T - R)).clamp_(0, 1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detail_bench.py needs a GPU: there is no CPU path to time")
    N, H, W = a.frames, a.height, a.width
    g = torch.Generator(device="cuda").manual_seed(1)
    S = torch.rand(N, 3, H, W, device="cuda", generator=g)
    R = (0.7 * S + 0.3 * torch.rand(N, 3, H, W, device="cuda", generator=g)).clamp_(0, 1)
    must = 36 * N * H * W
    variants, lines = [], []
    for sigma in (3.0, 16.0):
        taps = detail.gaussian_taps(sigma)[0].cuda()
        for mode in detail.MODES:
            hip = lambda s=sigma, m=mode: detail.detail_transfer(S, R, s, m, 1.0, "rgb")
            ref = lambda t=taps, m=mode: torch_detail(S, R, t, m, 1.0)
            d = (hip() - ref()).abs().max().item()
            variants += [(f"hip   sigma {sigma:4.1f} {mode:5s}", hip, d), (f"torch sigma {sigma:4.1f} {mode:5s}", ref, d)]
    for _, fn, _ in variants:                                    # warm-up of every shape the timed window uses
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(ROUNDS):                                      # alternating rounds
        for name, fn, _ in variants:
            times[name].append(timed(fn))
    lines.append(f"detail transfer, {N} frames of {W}x{H}, channels rgb, no mask; {ROUNDS} alternating rounds of {REPS} calls after a warm-up; "
                 f"device {torch.cuda.get_device_name(0)}")
    lines.append(f"bytes the algorithm must touch: 36 B per pixel = {must / 1e9:.3f} GB per call")
    lines.append(f"{'variant':28s} {'ms per call (median)':>22s} {'min .. max':>20s} {'GB/s of the must-touch bytes':>30s} {'max |hip - torch|':>18s}")
    for name, _, d in variants:
        t = sorted(times[name])
        med = t[len(t) // 2]
        lines.append(f"{name:28s} {med:22.3f} {t[0]:9.3f} .. {t[-1]:7.3f} {must / med / 1e6:30.1f} {d:18.2e}")
    for k in range(0, len(variants), 2):
        h, t = sorted(times[variants[k][0]]), sorted(times[variants[k + 1][0]])
        lines.append(f"{variants[k][0][6:]}: torch / hip = {t[len(t) // 2] / h[len(h) // 2]:.2f} (worst hip round against best torch round: {t[0] / h[-1]:.2f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
