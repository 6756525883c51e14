"""frame-lpips (tc_light_amd.evaluate.frame_lpips on lpips.LPIPSEngine) on a pair of random videos, timed: seeded stand-in weights, random uint8 frames.
python tools/micro/lpips_bench.py [--frames 300] [--height 720] [--width 1280] [--batch 4]
Every batch size the timed call uses is warmed up first (the convolutions' tile choice is timed on the first call of a shape).  Under
`rocprofv3 --kernel-trace --stats` (a run of its own) the kernel table shows where the time goes; the wall time printed then includes the tracing."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    from tc_light_amd.evaluate import frame_lpips
    from tc_light_amd.lpips import LPIPSEngine, seeded_state
    if not torch.cuda.is_available():
        raise RuntimeError("lpips_bench.py times the GPU engine and found no GPU")
    g = np.random.default_rng(0)
    edit = torch.from_numpy(g.integers(0, 256, (a.frames, a.height, a.width, 3), dtype=np.uint8))
    source = torch.from_numpy(g.integers(0, 256, (a.frames, a.height, a.width, 3), dtype=np.uint8))
    eng = LPIPSEngine(seeded_state(), "cuda")
    pairs = a.frames - 1
    for b in sorted({min(a.batch, pairs), pairs % a.batch or a.batch}):                 # the full batch and the last, shorter one
        frame_lpips(edit[:b + 1], source[:b + 1], eng, batch=b)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    mean, per = frame_lpips(edit, source, eng, batch=a.batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    flop = 2 * 9 * sum(ci * co * (a.height >> k) * (a.width >> k) for k, ci, co in
                       ((0, 3, 64), (0, 64, 64), (1, 64, 128), (1, 128, 128), (2, 128, 256), (2, 256, 256), (2, 256, 256), (3, 256, 512), (3, 512, 512),
                        (3, 512, 512), (4, 512, 512), (4, 512, 512), (4, 512, 512)))
    total = flop * 2 * pairs
    print(f"frame-lpips {a.frames} frames {a.width}x{a.height}, batch {a.batch}: {dt:.3f} s for {pairs} pairs, {1e3 * dt / pairs:.2f} ms/pair; convolution "
          f"arithmetic {flop / 1e12:.3f} TFLOP per image, {total / 1e12:.0f} TFLOP in all = {total / dt / 1e12:.0f} TFLOP/s over the wall time (frames uploaded from "
          f"host memory inside it); peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB; figure {mean:.6f}, finite {bool(np.isfinite(per).all())}")


if __name__ == "__main__":
    main()
