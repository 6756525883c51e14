"""Micro-benchmark of generation.keyframes: the two kernels alone, 60 frames of 1280x720 at interval 4 (16 keys, 44 frames in between), smooth random
flows below 2 px so the taps leave their pixel's own cache line as they do on a real clip.

Each entry is warmed up, then the two take turns for ROUNDS rounds; a round times REPS passes over all batches of the clip between device events.
Reported per entry: the median round's time per clip, the spread (min .. max over the rounds), and GB/s over the traffic model of csrc/keyframe.hip --
chain: 40 B per pixel and (frame, direction, distance) job, 28 B at distance 1 (no previous chain); propagate: 96 B per pixel of a frame in between,
24 B per pixel of a key frame (copied).  A device-to-device copy of the same bytes on the same box stands beside them, and the share of the 8 000 GB/s HBM peak that bench.py's rooflines
(roofline_path2, roofline_flow_ids) are measured against.

  python tools/micro/keyframe_bench.py [--frames 60] [--interval 4] [--out profiles/keyframe_60x1280x720.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tc_light_amd import hostlogic as HL, keyframe              # noqa: E402
from tc_light_amd.lib import lib, stream                        # noqa: E402

ROUNDS, REPS = 7, 3
HBM_PEAK_GBS = 8000.0             # the `peak` of bench.py's HBM-bound rooflines


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--interval", type=int, default=4)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "keyframe_bench.py measures on the GPU"
    N, K, H, W = a.frames, a.interval, a.height, a.width
    keys = HL.keyframe_ids(N, K)
    M = len(keys)
    g = torch.Generator(device="cuda").manual_seed(0)
    up = lambda t: torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=True).contiguous()
    # one smooth texture for all frames (neighbours 2 px apart differ by a few hundredths: the photometric gate stays open, as on a real clip)
    S = up(torch.rand(1, 3, H // 80, W // 80, device="cuda", generator=g)).repeat(N, 1, 1, 1).contiguous()
    R = torch.rand(M, 3, H, W, device="cuda", generator=g)
    fut = up(torch.rand(N, 2, H // 40, W // 40, device="cuda", generator=g) * 4 - 2)
    past = (-fut.roll(1, 0)).contiguous()
    fut[-1] = 0; past[0] = 0
    L = lib()
    h_keys, h_left, h_right, h_tw = keyframe.tables(keys, N)
    ws_bytes = L.tcl_keyframe_workspace_bytes(N, H, W, K)
    ws = torch.empty(ws_bytes // 4, device="cuda")
    out = torch.empty_like(S)
    holes = torch.empty(N, dtype=torch.int32, device="cuda")
    batches = keyframe.batches(keys)

    def chain():
        for g0, g1 in batches:
            L.tcl_flow_chain_f32(fut, past, h_keys, M, g0, g1, N, H, W, 0.1, ws, ws_bytes, stream())

    def prop():                                                  # on the chains the last batch left: the same gathers, whatever batch they belong to
        for g0, g1 in batches:
            L.tcl_keyframe_propagate_f32(S, R, out, holes, h_keys, M, g0, g1, h_left, h_right, h_tw, N, H, W, 0.1, 1.0 / 64, ws, ws_bytes, stream())

    gaps = [b - a_ for a_, b in zip(keys, keys[1:])]
    jobs1 = 2 * sum(1 for d in gaps if d > 1)
    jobs = 2 * sum(d - 1 for d in gaps)
    chain_bytes = (28 * jobs1 + 40 * (jobs - jobs1)) * H * W
    n_between = N - M
    keys_written = sum(g1 - g0 + 1 for g0, g1 in batches)
    prop_bytes = (96 * n_between + 24 * keys_written) * H * W
    src, dst = torch.empty(prop_bytes // 8, device="cuda"), torch.empty(prop_bytes // 8, device="cuda")      # copy: reads n, writes n = prop_bytes
    variants = [("tcl_flow_chain_f32", chain, chain_bytes), ("tcl_keyframe_propagate_f32", prop, prop_bytes),
                ("device copy of the same bytes", lambda: dst.copy_(src), prop_bytes)]
    for _, fn, _ in variants:
        fn(); fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(ROUNDS):
        for name, fn, _ in variants:
            times[name].append(timed(fn))
    chain(); prop(); torch.cuda.synchronize()
    share = int(holes.sum().item()) / (n_between * H * W)
    lines = [f"keyframe kernels alone: {N} frames of {W}x{H}, interval {K}: {M} keys, {n_between} frames in between, {len(batches)} batches, "
             f"workspace {ws_bytes / 2 ** 20:.0f} MiB, holes {share:.4f} of the pixels in between; {ROUNDS} alternating rounds of {REPS} passes",
             f"device: {torch.cuda.get_device_name(0)}"]
    for name, _, nbytes in variants:
        t = sorted(times[name])
        med = t[len(t) // 2]
        lines.append(f"{name:32s} {med:8.3f} ms per clip (min {t[0]:.3f} .. max {t[-1]:.3f}), {nbytes / 1e9:.2f} GB modelled, {nbytes / med / 1e6:8.1f} GB/s "
                     f"= {nbytes / med / 1e6 / HBM_PEAK_GBS:.2f} of the {HBM_PEAK_GBS:.0f} GB/s peak of bench.py's rooflines")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
