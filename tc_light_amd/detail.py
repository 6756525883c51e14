"""generation.detail_transfer on the device: the relit frames keep their low frequencies (the new light), the source frames give back the high ones.

gaussian_taps builds the tap table on the host (float64, rounded once to f32); detail_transfer checks shapes, dtypes and contiguity, allocates the
f32 workspace and issues tcl_detail_transfer_f32 (csrc/detail.hip; the arithmetic is spelled out at its prototype in include/tclight_hip.h).  There is
no torch arithmetic on the data path and no fallback.
"""
import math
import re

import numpy as np
import torch

from .hostlogic import DETAIL_CHANNELS as CHANNELS, DETAIL_MODES as MODES, DETAIL_SIGMA
from .lib import HEADER, lib, stream

SIGMA_MIN, SIGMA_MAX = DETAIL_SIGMA


def _header_constants():
    src = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+TCL_DETAIL_(\w+)\s+(\d+)", src)}


_C = _header_constants()
ROW_SEG, TILE_W, TILE_H, MAX_RADIUS = _C["ROW_SEG"], _C["TILE_W"], _C["TILE_H"], _C["MAX_RADIUS"]      # the kernels' segment / tile: edge cases of the tests


def radius_of(sigma):
    return int(math.ceil(3.0 * float(sigma)))


def gaussian_taps(sigma):
    """-> (taps [2r + 1] f32 on the host, r): w_k = exp(-k^2 / (2 sigma^2)) / sum for k = -r .. r with r = ceil(3 sigma), in float64, rounded once."""
    sigma = float(sigma)
    if not SIGMA_MIN <= sigma <= SIGMA_MAX:
        raise ValueError(f"detail transfer: sigma {sigma!r} outside [{SIGMA_MIN}, {SIGMA_MAX}]")
    r = radius_of(sigma)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return torch.from_numpy((w / w.sum()).astype(np.float32)), r


def _check(name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}, contiguous={t.is_contiguous()}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"detail transfer: {name} is {what}; expected a contiguous device f32 tensor of shape {tuple(shape)}")


def detail_transfer(source, relit, sigma=3.0, mode="add", blend=1.0, channels="rgb", mask=None):
    """source, relit [N,3,H,W] f32 in [0,1] on the device, mask [N,1,H,W] f32 in [0,1] or None -> the relit frames with the source's detail, a new
    [N,3,H,W] f32 tensor.  blend 0 launches nothing and returns `relit` itself."""
    if mode not in MODES:
        raise ValueError(f"detail transfer: mode {mode!r}, expected one of {' | '.join(MODES)}")
    if channels not in CHANNELS:
        raise ValueError(f"detail transfer: channels {channels!r}, expected one of {' | '.join(CHANNELS)}")
    blend = float(blend)
    if not 0.0 <= blend <= 1.0:
        raise ValueError(f"detail transfer: blend {blend!r} outside [0, 1]")
    taps, r = gaussian_taps(sigma)
    if not torch.is_tensor(relit) or relit.dim() != 4 or relit.shape[1] != 3:
        raise ValueError(f"detail transfer: relit frames {tuple(relit.shape) if torch.is_tensor(relit) else type(relit).__name__}, expected [N,3,H,W]")
    N, _, H, W = relit.shape
    _check("relit", relit, (N, 3, H, W))
    _check("source", source, (N, 3, H, W))
    if mask is not None:
        _check("mask", mask, (N, 1, H, W))
    if r > min(H, W) - 1:
        raise ValueError(f"detail transfer: sigma {float(sigma)} has radius {r}, more than min(H, W) - 1 = {min(H, W) - 1} of {H}x{W} frames")
    if blend == 0.0:
        return relit
    L = lib()
    m, luma = MODES.index(mode), CHANNELS.index(channels)
    ws_bytes = L.tcl_detail_transfer_workspace_bytes(N, H, W, m, luma)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=relit.device)
    out = torch.empty_like(relit)
    L.tcl_detail_transfer_f32(source, relit, 0 if mask is None else mask, out, N, H, W, taps, taps.numel(), r, m, luma, blend, ws, ws_bytes, stream())
    return out
