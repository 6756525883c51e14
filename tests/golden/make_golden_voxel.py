"""Generate tests/golden/voxel.npz by RUNNING THE REFERENCE's own `utils.general_utils.voxelization` (general_utils.py:222-256) on the CPU.

Needs the reference checkout (TCL_REFERENCE, default /root/reference); only the .npz and this script are committed.  The reference module is
imported in place with the stubs of the other make_golden* scripts (torchvision is never called by voxelization); `torch_scatter.scatter` is
not installed and is shimmed as what it computes on the CPU for reduce='mean': a sequential index_add_ followed by a division by the count
clamped to 1.

Three cases, each 4 frames of 12x16 with a synthetic track layout (ids pairwise distinct inside a frame, most pixels inherit an id of the
previous frame, mean colours and positions that collide in voxels):
  vox        voxel_size set
  vox_inst   the same with instance_ids
  inst_only  voxel_size=None with instance_ids
Recorded: flow_ids [M], rgb [M,3], xyz [M,3], instance [M], voxel_size, and the reference's unq_inv per case.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TCL_REFERENCE", "/root/reference")
N, H, W = 4, 12, 16
VOXEL = 0.25


def import_voxelization():
    sys.path.insert(0, REF)
    ts = types.ModuleType("torch_scatter")

    def scatter(src, index, dim=0, reduce="mean"):
        assert dim == 0 and reduce == "mean"
        k = int(index.max()) + 1
        s = torch.zeros(k, *src.shape[1:], dtype=src.dtype).index_add_(0, index, src)
        c = torch.zeros(k, dtype=src.dtype).index_add_(0, index, torch.ones(index.numel(), dtype=src.dtype)).clamp(min=1)
        return s / c.view(-1, *([1] * (src.dim() - 1)))
    ts.scatter = scatter
    sys.modules["torch_scatter"] = ts
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms})
    return importlib.import_module("utils.general_utils").voxelization


def layout(seed):
    """-> flow_ids int32 [N,H,W] (dense, distinct inside a frame), rgb [N,3,H,W], xyz [N,3,H,W], instance int64 [N,H,W]."""
    g = np.random.default_rng(seed)
    P = H * W
    ids = np.zeros((N, P), np.int32)
    ids[0] = g.permutation(P)
    nxt = P
    for f in range(1, N):
        keep = g.random(P) < 0.7
        perm = g.permutation(P)                          # pixel p inherits the id of pixel perm[p] of the previous frame: still distinct
        ids[f] = ids[f - 1][perm]
        fresh = np.flatnonzero(~keep)
        ids[f][fresh] = nxt + np.arange(fresh.size)
        nxt += fresh.size
    k = nxt
    # per-track colour / position on a coarse lattice plus a small per-observation jitter: several tracks share a voxel, the means stay inside it
    base_rgb = (g.integers(0, 2, (k, 3)) * (8 / 255) + 1 / 255).astype(np.float32)
    base_xyz = (g.integers(-1, 2, (k, 3)) * VOXEL * 2 + VOXEL * 0.5).astype(np.float32)
    rgb = base_rgb[ids] + g.uniform(-0.4, 0.4, (N, P, 3)).astype(np.float32) / 255
    xyz = base_xyz[ids] + g.uniform(-0.2, 0.2, (N, P, 3)).astype(np.float32) * VOXEL
    inst = g.integers(0, 3, (N, P)).astype(np.int64)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.reshape(N, H, W, 3).transpose(0, 3, 1, 2)))
    return torch.from_numpy(ids.reshape(N, H, W)), to(rgb), to(xyz), torch.from_numpy(inst.reshape(N, H, W))


def main():
    vox = import_voxelization()
    ids, rgb, xyz, inst = layout(20)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 3).contiguous()
    out = dict(flow_ids=ids.numpy(), rgb=rgb.numpy(), xyz=xyz.numpy(), instance=inst.numpy(), voxel_size=np.float64(VOXEL))
    for name, vs, use_inst in (("vox", VOXEL, False), ("vox_inst", VOXEL, True), ("inst_only", None, True)):
        inv = vox(ids.reshape(-1, 1).clone(), rows(rgb).clone(), rows(xyz).clone(), vs, instance_ids=inst.reshape(-1, 1) if use_inst else None)
        out[name + "_inv"] = inv.numpy().astype(np.int32)
        print(name, "voxels", int(inv.max()) + 1, "of", int(ids.max()) + 1, "tracks")
    np.savez_compressed(os.path.join(HERE, "voxel.npz"), **out)


if __name__ == "__main__":
    main()
