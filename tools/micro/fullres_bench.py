"""Micro-benchmark of generation.fullres: 60 frames of 1280x720 applied to 3840x2160, the two HIP entries each on its own, then the whole step as
run.py performs it (fullres.fullres: batches under the device cap, the native crop up, the result down, assembled on the host; no file is written).

Every variant is warmed up, then the variants take turns for ROUNDS rounds; a round times REPS back-to-back calls between device events.  Reported per
variant: the median round's time per call, the spread (min .. max over the rounds), and GB/s over the bytes the algorithm must move:
  fit    S and R read, abar and bbar written: 48 B per working pixel; beside them the f32 workspace -- 12 planes of moment row sums (8 under luma), 6 of
         a and b and 6 of their row sums, each written once and read once: 192 B per working pixel (160 under luma), reported as its own column;
  apply  3 B read + 3 B written per output pixel; the fields (24 B per working pixel) come through L2.
The whole step is timed with the host clock around a synchronised call, once warm.

  python tools/micro/fullres_bench.py [--frames 60] [--out profiles/fullres_60x1280x720.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tc_light_amd import fullres                                # noqa: E402

ROUNDS, REPS = 7, 5


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
    ap.add_argument("--scale", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fullres_bench.py needs a GPU: there is no CPU path to time")
    N, h, w = a.frames, a.height, a.width
    Hc, Wc = a.scale * h, a.scale * w
    g = torch.Generator(device="cuda").manual_seed(1)
    S = torch.rand(N, 3, h, w, device="cuda", generator=g)
    R = (0.7 * S + 0.3 * torch.rand(N, 3, h, w, device="cuda", generator=g)).clamp_(0, 1)
    native = torch.randint(0, 256, (N, Hc, Wc, 3), device="cuda", generator=g, dtype=torch.uint8)
    abar, bbar = fullres.guided_fit(S, R, 8, 1e-3, "rgb")
    px, opx = N * h * w, N * Hc * Wc
    variants = [("fit   rgb  r  8", lambda: fullres.guided_fit(S, R, 8, 1e-3, "rgb"), 48 * px, 192 * px),
                ("fit   luma r  8", lambda: fullres.guided_fit(S, R, 8, 1e-3, "luma"), 48 * px, 160 * px),
                ("fit   rgb  r 64", lambda: fullres.guided_fit(S, R, 64, 1e-3, "rgb"), 48 * px, 192 * px),
                (f"apply {a.scale}x", lambda: fullres.guided_apply(abar, bbar, native), 6 * opx, 24 * px)]
    for _, fn, _, _ in variants:                                 # warm-up of every shape the timed window uses
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in variants}
    for _ in range(ROUNDS):                                      # alternating rounds
        for name, fn, _, _ in variants:
            times[name].append(timed(fn))
    lines = [f"full-resolution output, {N} frames of {w}x{h} -> {Wc}x{Hc}; {ROUNDS} alternating rounds of {REPS} calls after a warm-up; "
             f"device {torch.cuda.get_device_name(0)}",
             f"{'variant':18s} {'ms per call (median)':>22s} {'min .. max':>20s} {'must-move GB':>14s} {'GB/s of them':>14s} {'+ workspace / L2 GB':>20s} "
             f"{'GB/s with them':>16s}"]
    for name, _, must, extra in variants:
        t = sorted(times[name])
        med = t[len(t) // 2]
        lines.append(f"{name:18s} {med:22.3f} {t[0]:9.3f} .. {t[-1]:7.3f} {must / 1e9:14.3f} {must / med / 1e6:14.1f} {extra / 1e9:20.3f} "
                     f"{(must + extra) / med / 1e6:16.1f}")
    host = native.cpu()
    del native
    whole = []
    for _ in range(3):                                           # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fullres.fullres(S, R, host, 8, 1e-3, "rgb")
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    B = fullres.batch_size(h, w, Hc, Wc)
    lines.append(f"the whole step (fullres.fullres, rgb r 8, batches of {B} frames under the {fullres.CAP_BYTES >> 20} MiB cap, native frames from the host "
                 f"and the result back to it): {min(whole[1:]):.3f} s warm ({whole[0]:.3f} s the first time), {min(whole[1:]) / N * 1e3:.1f} ms per frame; "
                 f"output {tuple(out.shape)} uint8")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
