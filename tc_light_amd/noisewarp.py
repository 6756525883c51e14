"""generation.noise_mode warp on the device: the noise of a clip is a pixel-resolution field carried from frame to frame along the backward optical flow
-- the same where nothing moves, following the surface where it moves, fresh where something is uncovered, white and unit-variance in every frame; a
frame's latent noise is the normalised 8 x 8 block sum of its field.

warp_chain checks shapes, dtypes, devices and contiguity, and issues tcl_noise_warp_count and tcl_noise_warp_apply_f32 frame by frame (csrc/noisewarp.hip;
the arithmetic is spelled out at the prototypes in include/tclight_hip.h).  Two fields (ping-pong) and the workspace are held, whatever the clip's
length.  There is no torch arithmetic on the data path and no fallback.
"""
import torch

from .lib import lib, stream

CELL = 8      # TCL_NOISE_WARP_CELL: pixels per latent sample and axis


def _check(name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}, contiguous={t.is_contiguous()}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"noise_mode warp: {name} is {what}; expected a contiguous device f32 tensor of shape {tuple(shape)}")


def field_draw(rng, dev):
    """The G_draw of warp_chain the Generator uses: one torch.randn(4, H, W) call per frame from `rng`, so neither batching nor the number of ranks
    changes the stream."""
    return lambda H, W: torch.randn(4, H, W, generator=rng, device=dev, dtype=torch.float32)


def warp_chain(G_draw, past_flows, mask_bwds, n_total, H, W):
    """G_draw(H, W) -> the fresh field [4,H,W] f32 of the next frame (called once per frame, in frame order); past_flows [n_total,2,H,W] (frame t to
    t-1), mask_bwds [n_total,1,H,W], f32 on the device -> z [n_total,4,H/8,W/8] f32, the latent noise of every frame.  Sequential over the frames:
    at most three launches each (workspace clear, count, apply)."""
    n_total, H, W = int(n_total), int(H), int(W)
    if n_total < 1 or H < CELL or W < CELL or H % CELL or W % CELL:
        raise ValueError(f"noise_mode warp: {n_total} frames of {H}x{W}; expected at least one frame and sides that are multiples of {CELL}")
    _check("past_flows", past_flows, (n_total, 2, H, W))
    _check("mask_bwds", mask_bwds, (n_total, 1, H, W))
    if past_flows.device != mask_bwds.device:
        raise ValueError("noise_mode warp: past_flows and mask_bwds must live on one device")
    L, dev = lib(), past_flows.device
    ws_bytes = L.tcl_noise_warp_workspace_bytes(H, W)
    if ws_bytes == 0:
        raise ValueError(f"noise_mode warp: {H}x{W} is outside what tcl_noise_warp_count takes")
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    fields = [torch.empty(4, H, W, dtype=torch.float32, device=dev) for _ in range(2)]
    z = torch.empty(n_total, 4, H // CELL, W // CELL, dtype=torch.float32, device=dev)
    for t in range(n_total):
        G = G_draw(H, W)
        _check("the drawn field", G, (4, H, W))
        prev, cur = fields[(t + 1) & 1], fields[t & 1]
        if t > 0:
            L.tcl_noise_warp_count(past_flows, mask_bwds, G, t, n_total, H, W, ws, ws_bytes, stream())
        L.tcl_noise_warp_apply_f32(past_flows, mask_bwds, G, prev, cur, z, t, n_total, H, W, ws, ws_bytes, stream())
    return z
