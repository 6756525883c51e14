"""NumPy / float64 restatements of what the background-conditioned IC-Light model (generation.iclight_model: fbc) adds: the background ramps, the
grey matte of the foreground and the 12-channel input assembly.  The kernels' arithmetic is restated here from the header's comments, never from
the kernels' outputs."""
import numpy as np
import torch

# bg_source -> (axis, first sample, last sample): IC-Light's background demo, restated in DESIGN section 6
RAMPS = {"left": ("x", 224, 32), "right": ("x", 32, 224), "top": ("y", 224, 32), "bottom": ("y", 32, 224), "grey": ("x", 64, 64)}


def linspace_u8(start, stop, n):
    """uint8(np.linspace(start, stop, n)) by the documented rule, every operation in f64: start + k*step, step = (stop - start)/(n - 1), the last
    sample = stop, n == 1 -> start; truncated."""
    start, stop = np.float64(start), np.float64(stop)
    if n == 1:
        return np.array([int(start)], dtype=np.uint8)
    step = (stop - start) / np.float64(n - 1)
    v = np.arange(n, dtype=np.float64) * step + start
    v[-1] = stop
    return v.astype(np.int64).astype(np.uint8)


def ramp_u8(source, H, W):
    """[H,W] uint8 plane of bg_source left | right | top | bottom | grey."""
    axis, start, stop = RAMPS[source]
    if axis == "x":
        return np.tile(linspace_u8(start, stop, W)[None, :], (H, 1))
    return np.tile(linspace_u8(start, stop, H)[:, None], (1, W))


def matte_q(f, a):
    """The integer the matte stores, per element in f32 with every operation rounded on its own: u = 255 f; v = 127 + (u - 127) a;
    q = trunc(clamp(v, 0, 255)).  f, a: arrays broadcast against each other."""
    f, a = np.asarray(f, dtype=np.float32), np.asarray(a, dtype=np.float32)
    u = (np.float32(255.0) * f).astype(np.float32)
    d = (u - np.float32(127.0)).astype(np.float32)
    m = (d * a).astype(np.float32)
    v = (np.float32(127.0) + m).astype(np.float32)
    return np.trunc(np.clip(v, np.float32(0.0), np.float32(255.0))).astype(np.int64)


def pack12(x, fg, bg, idx, mode, sl=0, nwin=0):
    """torch indexing restatement of tcl_pack_latents12_f16: x / fg [N,4,h,w], bg [1|N,4,h,w] -> [2F,H',W',12] (both CFG halves)."""
    N = x.shape[0]
    full = torch.cat([x, fg, bg.expand(N, -1, -1, -1)], dim=1)           # [N,12,h,w]
    idx = torch.as_tensor(idx, dtype=torch.long)
    if mode == 0:
        one = full[idx].permute(0, 2, 3, 1)                              # [F,h,w,12]
    else:
        one = full[sl:sl + nwin][:, :, :, idx].permute(3, 0, 2, 1)       # 'n c h w -> w n h c'
    return torch.cat([one, one]).contiguous()
