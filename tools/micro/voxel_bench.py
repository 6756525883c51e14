"""Time tc_light_amd.voxel.voxelization (csrc/voxel.hip) at 60 frames of 960x540 against the plain composition a port would use on the same
inputs (device torch.unique(dim=0) on the float key rows + index_add_), and the box's flash-attention-alone rate (bench.py's `roofline.alone`
figure, same shape) so that runs on different boxes can be compared.

Inputs: a translating, colour-quantised synthetic plane (tests/synth.py), analytic flows, ids from the engine's get_flowid; world pitch 0.01 per
pixel, voxel_size 0.03.  Both chains are warmed up, then timed alternately (`--repeats` rounds of `--calls` calls, host clock around a device
synchronise; every call ends in a device-to-host read of the count, as the product call does).  Bytes moved = the bytes the algorithm has to
touch once (rgb + xyz + ids read, inv written), not the traffic of the kernels.
    python tools/micro/voxel_bench.py [--frames 60 --height 540 --width 960] [--once]    (--once: one call of the HIP chain, for a profiler)
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_inputs(n, h, w, dev, sx=2, sy=1, pitch=0.01):
    import synth
    from tc_light_amd.flow_ids import get_flowid, get_soft_mask_bwds
    base = synth.video_clip(1, h + sy * n, w + sx * n, seed=5, shift=(0, 0), jitter=0.0)["frames"][0]
    base = (torch.floor(base * 4) / 4 + 0.1).clamp(0, 1)
    fr = torch.stack([base[:, k * sy:k * sy + h, k * sx:k * sx + w] for k in range(n)]).contiguous().to(dev)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    xyz = torch.stack([torch.stack([(xs + k * sx) * pitch, (ys + k * sy) * pitch, torch.full((h, w), -3.0, device=dev)]) for k in range(n)]).float().contiguous()
    past = torch.zeros(n, 2, h, w, device=dev); past[1:, 0] = sx; past[1:, 1] = sy
    fut = torch.zeros(n, 2, h, w, device=dev); fut[:-1, 0] = -sx; fut[:-1, 1] = -sy
    masks = get_soft_mask_bwds(fr, fut, past, alpha=0.1)
    ids, k = get_flowid(fr, fut, masks)
    return fr, xyz, ids.reshape(-1), k


def torch_chain(ids, rgb_rows, xyz_rows, voxel_size, k):
    """voxelization as the reference writes it, on the device with torch primitives (scatter-mean as index_add_ / count)."""
    idx = ids.long()
    cnt = torch.zeros(k, device=ids.device).index_add_(0, idx, torch.ones(idx.numel(), device=ids.device)).clamp_(min=1)
    m_rgb = torch.zeros(k, 3, device=ids.device).index_add_(0, idx, rgb_rows) / cnt[:, None]
    m_xyz = torch.zeros(k, 3, device=ids.device).index_add_(0, idx, xyz_rows) / cnt[:, None]
    m_rgb = m_rgb.div_(2 / 255, rounding_mode="floor")
    m_xyz -= m_xyz.min(dim=0).values[None, :]
    m_xyz = m_xyz.div_(torch.full((1, 3), voxel_size, device=ids.device), rounding_mode="floor")
    uq, inv = torch.unique(torch.cat([m_xyz, m_rgb], dim=1), return_inverse=True, dim=0)
    return inv[idx], uq.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--voxel_size", type=float, default=0.03)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no_flash_alone", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "voxel_bench needs a GPU"
    dev = torch.device("cuda:0")
    from tc_light_amd.voxel import voxelization
    n, h, w = a.frames, a.height, a.width
    fr, xyz, ids, k = make_inputs(n, h, w, dev)
    hip = lambda: voxelization(ids, fr, xyz, a.voxel_size, n, h, w)
    if a.once:
        hip(); torch.cuda.synchronize()
        inv, k2 = hip(); torch.cuda.synchronize()
        print(json.dumps({"tracks": k, "voxels": k2}))
        return
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 3).contiguous()
    rgb_rows, xyz_rows = rows(fr), rows(xyz)              # the port's layout, prepared outside its timed window
    ref = lambda: torch_chain(ids, rgb_rows, xyz_rows, a.voxel_size, k)
    (inv_h, k_h), (inv_t, k_t) = hip(), ref()
    hip(); ref(); torch.cuda.synchronize()
    # same partition?  (float atomics reorder the port's sums, so a few means may land in a neighbouring cell: report, do not assert)
    pair = torch.unique(torch.stack([inv_h.long(), inv_t.long()], dim=1), dim=0).shape[0]
    times = {"hip": [], "torch": []}
    for _ in range(a.repeats):
        for name, f in (("hip", hip), ("torch", ref)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.calls * 1e3)
    M = n * h * w
    nbytes = M * (12 + 12 + 4 + 4)
    res = {"shape": {"frames": n, "height": h, "width": w}, "pixels": M, "tracks": k, "voxels_hip": k_h, "voxels_torch": k_t,
           "distinct_label_pairs": pair, "bytes_algorithm": nbytes,
           "hip_ms": times["hip"], "torch_ms": times["torch"],
           "hip_ms_median": float(np.median(times["hip"])), "torch_ms_median": float(np.median(times["torch"])),
           "hip_GBps": nbytes / (float(np.median(times["hip"])) * 1e-3) / 1e9, "torch_GBps": nbytes / (float(np.median(times["torch"])) * 1e-3) / 1e9,
           "how": f"{a.repeats} alternating rounds of {a.calls} calls after warm-up, host clock around a device synchronise"}
    if not a.no_flash_alone:
        import bench
        res["roofline_alone"] = bench.flash_alone((2, 8, 47520, 47520), dev, n=20)["achieved"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
