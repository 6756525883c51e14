"""Spatio-temporal Unique Video Tensor, host side (reference: voxelization, utils/general_utils.py:222-256; kernels: csrc/voxel.hip).

Tracks (flow ids, optionally split by instance) whose MEAN colour and MEAN world position fall into the same colour-and-position voxel share one
codebook row.  Every step runs on the device: per-track means, quantisation, unique rows.  Ids are numbered by first appearance in row order (the
reference: lexicographic rank of the key rows) -- a permutation of codebook rows; stage 2 has no cross-row term, so the partition is what counts.
"""
import torch

from .lib import check, lib, stream

RGB_VOX_SIZE = 2 / 255                                   # general_utils.py:223


def unproject_sceneflow(depth, intrinsics, c2w):
    """rgbd2pcd (sceneflow_dataparsers.py:257-274): depth [N,H,W] f32, intrinsics (fx, fy, cx, cy), c2w [N,4,4] f32 -> p_world [N,3,H,W] f32."""
    depth, c2w = check(depth, torch.float32), check(c2w, torch.float32)
    n, h, w = depth.shape
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    out = torch.empty(n, 3, h, w, device=depth.device)
    lib().tcl_unproject_sceneflow(depth, c2w, n, h, w, fx, fy, cx, cy, out, stream())
    return out


def unique_rows(keys, ws=None):
    """torch.unique(keys, dim=0, return_inverse=True) on int32 rows [n,C], C <= 6 -> (inv int32 [n], count); first-appearance numbering."""
    keys = check(keys, torch.int32)
    n, c = keys.shape
    L = lib()
    nbytes = L.tcl_unique_rows_workspace_bytes(n)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=keys.device)
    inv = torch.empty(n, dtype=torch.int32, device=keys.device)
    count = torch.zeros(1, dtype=torch.int32, device=keys.device)
    L.tcl_unique_rows_i32(keys, n, c, inv, count, ws, stream())
    return inv, int(count.item())


def track_mean(values, ids, k):
    """torch_scatter.scatter(values, ids, reduce='mean'): values [N,C,H,W] f32 (C <= 3), ids [N,H,W] int32 in [0, k) -> (mean [k,C], cnt [k]).
    The ids of every frame must be pairwise distinct (checked on the device; ValueError otherwise): the sums then need no atomics and equal a
    sequential scatter in row order bit for bit."""
    from .post_opt import track_ids_unique
    values, ids = check(values, torch.float32), check(ids, torch.int32)
    n, c, h, w = values.shape
    if tuple(ids.shape) != (n, h, w):
        raise ValueError(f"ids {tuple(ids.shape)} do not match values {tuple(values.shape)}")
    if ids.min().item() < 0 or ids.max().item() >= k:
        raise ValueError(f"track ids must lie in [0, {k})")
    if not track_ids_unique(ids, n, h, w, k):
        raise ValueError("track_mean needs ids that are pairwise distinct inside every frame (true of get_flowid ids, also split by instance)")
    mean = torch.empty(k, c, device=values.device)
    cnt = torch.empty(k, device=values.device)
    lib().tcl_track_mean_f32(values, ids, n, c, h, w, k, mean, cnt, stream())
    return mean, cnt


def voxel_keys(mean_rgb, mean_xyz, xyz_min, voxel_size, rgb_vox_size=RGB_VOX_SIZE):
    """general_utils.py:238,243-250 -> keys int32 [K,6] = (floor_div(xyz - xyz_min, voxel_size) | floor_div(rgb, rgb_vox_size))."""
    mean_rgb, mean_xyz, xyz_min = check(mean_rgb, torch.float32), check(mean_xyz, torch.float32), check(xyz_min, torch.float32)
    k = mean_rgb.shape[0]
    keys = torch.empty(k, 6, dtype=torch.int32, device=mean_rgb.device)
    lib().tcl_voxel_keys(mean_rgb, mean_xyz, xyz_min, float(voxel_size), float(rgb_vox_size), k, keys, stream())
    return keys


def voxelization(flow_ids, rgb, xyz, voxel_size, n, h, w, instance_ids=None, contract=False):
    """voxelization (general_utils.py:222-256) -> (inv int32 [n*h*w], k).

    flow_ids: int32 [n*h*w] (any shape with that many entries), dense in [0, K), pairwise distinct inside a frame; rgb, xyz: [n,3,h,w] f32;
    instance_ids: integer tensor with n*h*w entries or None.  voxel_size None and no instance ids: the ids unchanged.  xyz_min is always the
    data's own (the reference never passes one).  contract=True (contract_to_unisphere, host histograms) is not built."""
    if contract:
        raise NotImplementedError("data.contract: contract_to_unisphere (general_utils.py:181-220) is not built in this engine")
    ids = flow_ids.reshape(-1)
    if ids.dtype != torch.int32:
        ids = ids.to(torch.int32)
    ids = ids.contiguous()
    if ids.numel() != n * h * w:
        raise ValueError(f"flow_ids has {ids.numel()} entries, expected {n}*{h}*{w}")
    if instance_ids is not None:                         # general_utils.py:228-230: unique rows of (flow_id, instance)
        inst = instance_ids.reshape(-1).to(device=ids.device).to(ids.dtype)
        ids, k = unique_rows(torch.stack([ids, inst], dim=1).contiguous())
    else:
        k = int(ids.max().item()) + 1
    if voxel_size is None:
        return ids, k
    ids3 = ids.view(n, h, w)
    m_rgb, _ = track_mean(rgb.float().contiguous(), ids3, k)
    m_xyz, _ = track_mean(xyz.float().contiguous(), ids3, k)
    xyz_min = m_xyz.min(dim=0).values.contiguous()       # exact in any order (plumbing)
    inv2, k2 = unique_rows(voxel_keys(m_rgb, m_xyz, xyz_min, voxel_size))
    return inv2[ids.long()], k2
