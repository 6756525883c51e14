"""generation.keyframes on the device: the frames between two relit key frames are their source frame times the keys' gain field relit / source,
carried along the chained optical flows and blended by distance.

propagate checks shapes, dtypes, devices and contiguity, builds the host tables (tables), allocates the bounded workspace and issues
tcl_flow_chain_f32 and tcl_keyframe_propagate_f32 batch by batch (csrc/keyframe.hip; the arithmetic is spelled out at the prototypes in
include/tclight_hip.h).  There is no torch arithmetic on the data path and no fallback.
"""
import re

import numpy as np
import torch

from .lib import HEADER, lib, stream


def _header_constants():
    src = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+TCL_KEYFRAME_(\w+)\s+(\d+)", src)}


_C = _header_constants()
TILE_W, TILE_H, MAX_GAP, BATCH_FRAMES = _C["TILE_W"], _C["TILE_H"], _C["MAX_GAP"], _C["BATCH_FRAMES"]      # the kernels' tile: edge cases of the tests


def tables(keys, n):
    """The host tables of the C entries for the key frames `keys` of an n-frame clip -> (h_keys int32 [M], h_left int32 [n], h_right int32 [n],
    h_tw f32 [2, n]): the index among the keys of the last key at or before / the first key at or after each frame, and the temporal weights
    ta = (b - i) / (b - a), tb = 1 - ta of its two keys' frames a, b, each computed in float64 and rounded once (a key frame: 1, 0)."""
    keys = [int(k) for k in keys]
    if not keys or keys[0] != 0 or keys[-1] != n - 1 or any(b <= a or b - a > MAX_GAP for a, b in zip(keys, keys[1:])):
        raise ValueError(f"keyframes: keys {keys} must increase strictly from 0 to {n - 1} in steps of at most {MAX_GAP}")
    k = np.asarray(keys, dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    left = np.searchsorted(k, i, side="right") - 1
    right = np.searchsorted(k, i, side="left")
    a, b = k[left].astype(np.float64), k[right].astype(np.float64)
    ta = np.where(left == right, 1.0, (b - i) / np.maximum(b - a, 1.0))
    tw = np.stack([ta, 1.0 - ta]).astype(np.float32)
    as_i32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32))
    return as_i32(k), as_i32(left), as_i32(right), torch.from_numpy(tw)


def batches(keys, slots=BATCH_FRAMES):
    """The gaps of the clip in batches of whole gaps [(g0, g1), ...] with keys[g1] - keys[g0] + 1 <= slots frames each: what one pair of calls covers."""
    out, g0, m = [], 0, len(keys)
    while g0 < m - 1:
        g1 = g0 + 1
        while g1 + 1 <= m - 1 and keys[g1 + 1] - keys[g0] + 1 <= slots:
            g1 += 1
        out.append((g0, g1))
        g0 = g1
    return out


def _check(name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}, contiguous={t.is_contiguous()}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"keyframes: {name} is {what}; expected a contiguous device f32 tensor of shape {tuple(shape)}")


def propagate(source, relit_keys, keys, fut, past, alpha=0.1, diff_threshold=0.1, eps=0.015625):
    """source [N,3,H,W] (all frames of the clip), relit_keys [M,3,H,W] (the relit frames `keys`, frame numbers increasing from 0 to N-1), fut / past
    [N,2,H,W] (frame i to i+1 / to i-1), all f32 on the device -> (frames [N,3,H,W] f32: the keys bit for bit, the others propagated; holes [N] int32:
    pixels per frame that neither key explains).  len(keys) == N launches nothing and returns `relit_keys` itself (holes all 0)."""
    if not torch.is_tensor(source) or source.dim() != 4 or source.shape[1] != 3:
        raise ValueError(f"keyframes: source frames {tuple(source.shape) if torch.is_tensor(source) else type(source).__name__}, expected [N,3,H,W]")
    N, _, H, W = source.shape
    keys = [int(k) for k in keys]
    for name, v in (("alpha", alpha), ("diff_threshold", diff_threshold)):
        if not 0.0 < float(v) < float("inf"):
            raise ValueError(f"keyframes: {name} {v!r} is not a number > 0")
    if not 0.0 < float(eps) <= 0.25:
        raise ValueError(f"keyframes: eps {eps!r} outside (0, 0.25]")
    h_keys, h_left, h_right, h_tw = tables(keys, N)
    M = len(keys)
    _check("source", source, (N, 3, H, W))
    _check("relit_keys", relit_keys, (M, 3, H, W))
    _check("fut", fut, (N, 2, H, W))
    _check("past", past, (N, 2, H, W))
    if any(t.device != source.device for t in (relit_keys, fut, past)):
        raise ValueError("keyframes: source, relit_keys, fut and past must live on one device")
    if M == N:
        return relit_keys, torch.zeros(N, dtype=torch.int32, device=source.device)
    L = lib()
    ws_bytes = L.tcl_keyframe_workspace_bytes(N, H, W, max(b - a for a, b in zip(keys, keys[1:])))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=source.device)
    out = torch.empty_like(source)
    holes = torch.empty(N, dtype=torch.int32, device=source.device)
    for g0, g1 in batches(keys):
        L.tcl_flow_chain_f32(fut, past, h_keys, M, g0, g1, N, H, W, float(alpha), ws, ws_bytes, stream())
        L.tcl_keyframe_propagate_f32(source, relit_keys, out, holes, h_keys, M, g0, g1, h_left, h_right, h_tw, N, H, W, float(diff_threshold),
                                     float(eps), ws, ws_bytes, stream())
    return out, holes
