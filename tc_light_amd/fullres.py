"""generation.fullres on the device: the relight applied to the source's own pixels (the fast guided filter, He & Sun 2015).

geometry() maps the working frame back to the native one; guided_fit / guided_apply check shapes, dtypes and contiguity and issue tcl_guided_fit_f32 /
tcl_guided_apply_u8 (csrc/guided.hip; the arithmetic is spelled out at their prototypes in include/tclight_hip.h); fullres() runs a whole clip in
batches under a device-memory cap and assembles the result on the host.  There is no torch arithmetic on the data path and no fallback.

Geometry.  dataparser.process_frames resizes a native H0 x W0 frame by s = max(w / W0, h / H0) to (nh, nw) = (round(H0 s), round(W0 s)) and crops
(h, w) out of it at (t, l) = (round((nh - h) / 2), round((nw - w) / 2)).  The native crop the working frame shows is
    X0 = round(l / s), Y0 = round(t / s), Wc = min(round(w / s), W0 - X0), Hc = min(round(h / s), H0 - Y0)
with round = Python's round (to nearest, ties to even) throughout, as process_frames uses it.  s >= 1 -- a source that is not larger than the working
size on the covering axis -- is refused: there is nothing to give back.
"""
import re

import numpy as np
import torch

from .hostlogic import FULLRES_DEFAULTS, FULLRES_EPS, FULLRES_GUIDES as GUIDES, FULLRES_RADIUS
from .lib import HEADER, lib, stream

CAP_BYTES = 1 << 30      # device bytes one batch may hold: source + output bytes, the two fields and the fit's workspace


def _header_constants():
    src = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+TCL_GUIDED_(\w+)\s+(\d+)", src)}


_C = _header_constants()
ROW_SEG, TILE_W, TILE_H, MAX_RADIUS, WS_PLANES = _C["ROW_SEG"], _C["TILE_W"], _C["TILE_H"], _C["MAX_RADIUS"], _C["WS_PLANES"]


def geometry(H0, W0, h, w):
    """Native size (H0, W0), working size (h, w) -> dict(s, nh, nw, t, l, X0, Y0, Hc, Wc): process_frames' numbers and the native crop (see above)."""
    H0, W0, h, w = int(H0), int(W0), int(h), int(w)
    if min(H0, W0, h, w) < 1:
        raise ValueError(f"generation.fullres: sizes {H0}x{W0} (source) and {h}x{w} (result) must be positive")
    s = max(w / W0, h / H0)
    if s >= 1.0:
        raise ValueError(f"generation.fullres: the source frames are {H0}x{W0}, not larger than the {h}x{w} result on the covering axis (scale "
                         f"{s:.4g} >= 1): there is no finer source to apply the relight to")
    nh, nw = int(round(H0 * s)), int(round(W0 * s))
    t, l = int(round((nh - h) / 2.0)), int(round((nw - w) / 2.0))
    X0, Y0 = int(round(l / s)), int(round(t / s))
    Wc, Hc = min(int(round(w / s)), W0 - X0), min(int(round(h / s)), H0 - Y0)
    return dict(s=s, nh=nh, nw=nw, t=t, l=l, X0=X0, Y0=Y0, Hc=Hc, Wc=Wc)


def _check(name, t, shape, dtype=torch.float32):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}, contiguous={t.is_contiguous()}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"fullres: {name} is {what}; expected a contiguous device {dtype} tensor of shape {tuple(shape)}")


def _options(radius, eps, guide):
    if isinstance(radius, bool) or not isinstance(radius, int) or not FULLRES_RADIUS[0] <= radius <= FULLRES_RADIUS[1]:
        raise ValueError(f"fullres: radius {radius!r}, expected an integer in [{FULLRES_RADIUS[0]}, {FULLRES_RADIUS[1]}]")
    if not FULLRES_EPS[0] <= float(eps) <= FULLRES_EPS[1]:
        raise ValueError(f"fullres: eps {eps!r} outside [{FULLRES_EPS[0]}, {FULLRES_EPS[1]}]")
    if guide not in GUIDES:
        raise ValueError(f"fullres: guide {guide!r}, expected one of {' | '.join(GUIDES)}")
    return radius, float(np.float32(eps)), GUIDES.index(guide)      # the kernel's f32 value of eps


def guided_fit(source, relit, radius=FULLRES_DEFAULTS["radius"], eps=FULLRES_DEFAULTS["eps"], guide=FULLRES_DEFAULTS["guide"]):
    """source, relit [N,3,h,w] f32 in [0,1] on the device -> (abar, bbar), both new [N,3,h,w] f32: relit ~ abar * source + bbar, smooth fields."""
    radius, eps, luma = _options(radius, eps, guide)
    if not torch.is_tensor(relit) or relit.dim() != 4 or relit.shape[1] != 3:
        raise ValueError(f"fullres: relit frames {tuple(relit.shape) if torch.is_tensor(relit) else type(relit).__name__}, expected [N,3,h,w]")
    N, _, h, w = relit.shape
    _check("relit", relit, (N, 3, h, w))
    _check("source", source, (N, 3, h, w))
    L = lib()
    ws_bytes = L.tcl_guided_workspace_bytes(N, h, w)
    if ws_bytes == 0:
        raise ValueError(f"fullres: {N} frames of {h}x{w} are more than one call takes (N <= 65535, N * {WS_PLANES} * h * w < 2^31): use fullres()'s batches")
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=relit.device)
    abar, bbar = torch.empty_like(relit), torch.empty_like(relit)
    L.tcl_guided_fit_f32(source, relit, abar, bbar, N, h, w, radius, eps, luma, ws, ws_bytes, stream())
    return abar, bbar


def guided_apply(abar, bbar, native):
    """abar, bbar [N,3,h,w] f32 and native [N,Hc,Wc,3] uint8, all on the device -> a new [N,Hc,Wc,3] uint8 tensor: the bilinearly upsampled fields
    applied to the native pixels, rounded to nearest and clamped."""
    if not torch.is_tensor(abar) or abar.dim() != 4 or abar.shape[1] != 3:
        raise ValueError(f"fullres: abar {tuple(abar.shape) if torch.is_tensor(abar) else type(abar).__name__}, expected [N,3,h,w]")
    N, _, h, w = abar.shape
    _check("abar", abar, (N, 3, h, w))
    _check("bbar", bbar, (N, 3, h, w))
    if not torch.is_tensor(native) or native.dim() != 4 or native.shape[0] != N or native.shape[3] != 3:
        raise ValueError(f"fullres: native frames {tuple(native.shape) if torch.is_tensor(native) else type(native).__name__}, expected [{N},Hc,Wc,3]")
    _check("native", native, native.shape, torch.uint8)
    out = torch.empty_like(native)
    lib().tcl_guided_apply_u8(abar, bbar, native, out, N, h, w, native.shape[1], native.shape[2], stream())
    return out


def bytes_per_frame(h, w, Hc, Wc):
    """Device bytes fullres() allocates per frame of a batch: the native crop and the output (uint8), abar and bbar, the fit's workspace."""
    return 2 * 3 * Hc * Wc + 2 * 3 * h * w * 4 + WS_PLANES * h * w * 4


def batch_size(h, w, Hc, Wc, cap_bytes=CAP_BYTES):
    """Frames per batch so that a batch stays under cap_bytes whatever the clip's length; one frame at least (a single frame above the cap still runs,
    alone) and no more than one fit call takes."""
    per_call = max(1, (2 ** 31 - 1) // (WS_PLANES * h * w))
    return max(1, min(int(cap_bytes) // bytes_per_frame(h, w, Hc, Wc), per_call, 65535))


def fullres(source, relit, native, radius=FULLRES_DEFAULTS["radius"], eps=FULLRES_DEFAULTS["eps"], guide=FULLRES_DEFAULTS["guide"], crop=None,
            cap_bytes=CAP_BYTES):
    """source, relit [N,3,h,w] f32 in [0,1] on the device (the source at the size of the result, and the result); native [N,H0,W0,3] uint8 on the HOST
    (the source frames as they were read); crop: (Y0, X0, Hc, Wc) of the native frames, None: all of them -> [N,Hc,Wc,3] uint8 on the host.  The
    frames go through the device in batches of batch_size(); every frame is on its own, so the batching changes no bit."""
    if not torch.is_tensor(native) or native.dtype != torch.uint8 or native.dim() != 4 or native.shape[3] != 3 or native.is_cuda:
        raise ValueError(f"fullres: native frames {tuple(native.shape) if torch.is_tensor(native) else type(native).__name__}, expected a host uint8 "
                         "tensor [N,H0,W0,3]")
    N, _, h, w = relit.shape
    if native.shape[0] != N:
        raise ValueError(f"fullres: {native.shape[0]} native frames for {N} relit frames")
    Y0, X0, Hc, Wc = (0, 0, native.shape[1], native.shape[2]) if crop is None else crop
    if Y0 < 0 or X0 < 0 or Hc < 1 or Wc < 1 or Y0 + Hc > native.shape[1] or X0 + Wc > native.shape[2]:
        raise ValueError(f"fullres: crop {crop} outside the native {native.shape[1]}x{native.shape[2]} frames")
    out = torch.empty(N, Hc, Wc, 3, dtype=torch.uint8)
    B = batch_size(h, w, Hc, Wc, cap_bytes)
    for lo in range(0, N, B):
        hi = min(lo + B, N)
        abar, bbar = guided_fit(source[lo:hi].contiguous(), relit[lo:hi].contiguous(), radius, eps, guide)
        nat = native[lo:hi, Y0:Y0 + Hc, X0:X0 + Wc].contiguous().to(relit.device)
        out[lo:hi] = guided_apply(abar, bbar, nat).cpu()
    return out
