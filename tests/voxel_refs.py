"""CPU references for the spatio-temporal Unique Video Tensor (csrc/voxel.hip, tc_light_amd/voxel.py), in torch and numpy.  Nothing here runs
the code under test: these are the yardsticks the GPU tests compare against."""
import numpy as np
import torch

RGB_VOX_SIZE = 2 / 255


def unproject_ref(depth, intrinsics, c2w):
    """rgbd2pcd in float64: depth [N,H,W], (fx, fy, cx, cy), c2w [N,4,4] -> (p_world [N,3,H,W] f64, bound [N,3,H,W] f64) where
    bound = |x||r0| + |y||r1| + |d||r2| + |t| per output component (the magnitude the rounding-error bound of the f32 sequence scales with)."""
    d = depth.double()
    c = c2w.double()
    n, h, w = d.shape
    fx, fy, cx, cy = (float(np.float32(v)) for v in intrinsics)
    px = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    py = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    x = (px - cx) * d / fx
    y = (py - cy) * d / fy
    hom = torch.stack([x, -y, -d, torch.ones_like(d)], dim=-1)                     # [N,H,W,4]
    out = torch.einsum("nhwk,njk->njhw", hom, c[:, :3, :])
    bound = torch.einsum("nhwk,njk->njhw", hom.abs(), c[:, :3, :].abs())
    return out, bound


def track_mean_ref(values, ids, k):
    """values [N,C,H,W] f32, ids [N,H,W] -> (mean [k,C] f32, cnt [k] f32): f32 sums in ROW order (frame, then pixel), then one division by
    max(cnt, 1).  index_add_ on the CPU is a sequential loop over the rows."""
    n, c, h, w = values.shape
    rows = values.float().permute(0, 2, 3, 1).reshape(-1, c).contiguous()
    idx = ids.reshape(-1).long()
    s = torch.zeros(k, c, dtype=torch.float32).index_add_(0, idx, rows)
    cnt = torch.zeros(k, dtype=torch.float32).index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float32))
    return s / cnt.clamp(min=1)[:, None], cnt


def floor_div_ref(a, b):
    """torch's own div(rounding_mode='floor') on float32 (a: tensor; b: tensor or Python scalar)."""
    return a.float().clone().div_(b, rounding_mode="floor")


def keys_ref(mean_rgb, mean_xyz, xyz_min, voxel_size, rgb_vox_size=RGB_VOX_SIZE):
    """-> int64 [K,6] (x, y, z, r, g, b), the float keys of general_utils.py:238-250 as integers (saturated to int32, NaN -> 0)."""
    xyz = mean_xyz.float() - xyz_min.float()[None, :]
    vs = torch.tensor([voxel_size] * 3, dtype=torch.float32)
    f = torch.cat([floor_div_ref(xyz, vs[None, :]), floor_div_ref(mean_rgb, rgb_vox_size)], dim=1)
    f = torch.nan_to_num(f, nan=0.0, posinf=2.0 ** 31, neginf=-2.0 ** 31)
    return f.double().clamp(-2.0 ** 31, 2.0 ** 31 - 1).long()


def voxelization_ref(flow_ids, rgb, xyz, voxel_size, instance_ids=None, rgb_vox_size=RGB_VOX_SIZE):
    """The reference's algorithm (general_utils.py:222-256) with torch.unique(dim=0).  flow_ids [M] ints, rgb / xyz [M,3] f32 rows (frame,
    pixel order), instance_ids [M] or None -> inv int64 [M] (lexicographic numbering)."""
    ids = flow_ids.reshape(-1, 1).cpu()
    if instance_ids is not None:
        ids = torch.cat([ids, instance_ids.reshape(-1, 1).cpu().to(ids.dtype)], dim=1)
    _, inv_t = torch.unique(ids, return_inverse=True, dim=0)
    if voxel_size is None:
        return inv_t
    k = int(inv_t.max()) + 1
    cnt = torch.zeros(k, dtype=torch.float32).index_add_(0, inv_t, torch.ones(inv_t.numel(), dtype=torch.float32)).clamp(min=1)
    m_rgb = torch.zeros(k, 3, dtype=torch.float32).index_add_(0, inv_t, rgb.float().cpu()) / cnt[:, None]
    m_xyz = torch.zeros(k, 3, dtype=torch.float32).index_add_(0, inv_t, xyz.float().cpu()) / cnt[:, None]
    m_rgb = m_rgb.div_(rgb_vox_size, rounding_mode="floor")
    m_xyz -= torch.min(m_xyz, dim=0).values[None, :]
    m_xyz = m_xyz.div_(torch.tensor([voxel_size] * 3, dtype=torch.float32)[None, :], rounding_mode="floor")
    _, inv_xyz = torch.unique(torch.cat([m_xyz, m_rgb], dim=1), return_inverse=True, dim=0)
    return inv_xyz[inv_t]


def canon(inv):
    """Renumber ids by first appearance: two labelings describe the same partition iff their canon() are equal.  -> int64 numpy [M]."""
    a = np.asarray(inv.cpu() if isinstance(inv, torch.Tensor) else inv).reshape(-1).astype(np.int64)
    _, first, back = np.unique(a, return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(first))                # rank of each distinct value by its first position
    return order[back.reshape(-1)]


def rows_nchw(t):
    """[N,C,H,W] -> [N*H*W, C] rows in (frame, pixel) order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
