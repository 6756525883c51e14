"""CPU restatement of the warp-error-ssim metric (evaluate.py's `SaveWarpingImage` with RAFT flows), written from its specification
("Evaluation"), numpy only.  float32 where the metric is float32 (the cubic remap, the consistency mask), float64 for SSIM.

  remap(img, flow)  : cubic remap of img [H,W,C] at x + flow, fixed point at 1/32 pixel (X = rint(m * 32), integer part X >> 5, fraction X & 31),
                      A = -0.75 weights, 2-D weight wy[i] * wx[j], taps from (ix - 1, iy - 1), taps outside the image read 0, summed row by row
  mask(fwd, bwd)    : |bwd + remap(fwd, bwd)| < 0.5 (|bwd| + |remap(fwd, bwd)|) + 0.5
  planes            : u8(where(mask, remap(edit_i, bwd), 0)), u8(where(mask, edit_i+1, 0)); u8 truncates toward zero and wraps modulo 256
  ssim(x, y)        : per channel 7x7 uniform window, sample covariance, data range 255, K1 0.01, K2 0.03, mean over the interior (3-pixel crop),
                      then the mean over the channels
"""
import numpy as np

F32 = np.float32
C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def cubic_weights(k):
    """A = -0.75 cubic weights at t = k / 32 (k integer array), float32: -> [..., 4]."""
    A = F32(-0.75)
    t = np.asarray(k, np.int64).astype(F32) * F32(1.0 / 32)
    x = t + F32(1)
    c0 = ((A * x - F32(5) * A) * x + F32(8) * A) * x - F32(4) * A
    c1 = ((A + F32(2)) * t - (A + F32(3))) * t * t + F32(1)
    x = F32(1) - t
    c2 = ((A + F32(2)) * x - (A + F32(3))) * x * x + F32(1)
    c3 = F32(1) - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], -1).astype(F32)


def fixed_point(m):
    """map coordinate (float32) -> (integer part, fraction index 0..31): X = rint(m * 32), round half to even."""
    X = np.clip(np.rint(m.astype(F32) * F32(32)), -1e9, 1e9).astype(np.int64)
    return X >> 5, X & 31


def remap(img, flow):
    """img [H,W,C] float32, flow [H,W,2] float32 -> [H,W,C] float32: img sampled at (x + flow_x, y + flow_y)."""
    img = np.asarray(img, F32)
    H, W, C = img.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mx = flow[..., 0].astype(F32) + xs.astype(F32)
    my = flow[..., 1].astype(F32) + ys.astype(F32)
    ix, fx = fixed_point(mx)
    iy, fy = fixed_point(my)
    wx, wy = cubic_weights(fx), cubic_weights(fy)
    acc = np.zeros((H, W, C), F32)
    for i in range(4):
        yy = iy - 1 + i
        row = np.zeros((H, W, C), F32)
        for j in range(4):
            xx = ix - 1 + j
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = np.where(ok[..., None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F32(0))
            w = (wy[..., i] * wx[..., j]).astype(F32)
            row = v * w[..., None] if j == 0 else row + v * w[..., None]
        acc = acc + row
    return acc


def consistency_mask(fwd, bwd, return_sides=False):
    """fwd, bwd [H,W,2] float32 -> bool [H,W]: the backward forward-backward check.  return_sides: also (lhs, rhs) of the comparison."""
    bwd = bwd.astype(F32)
    f2b = remap(fwd, bwd)
    e = bwd + f2b
    lhs = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1])
    n1 = np.sqrt(bwd[..., 0] * bwd[..., 0] + bwd[..., 1] * bwd[..., 1])
    n2 = np.sqrt(f2b[..., 0] * f2b[..., 0] + f2b[..., 1] * f2b[..., 1])
    rhs = F32(0.5) * (n1 + n2) + F32(0.5)
    m = lhs < rhs
    return (m, lhs, rhs) if return_sides else m


def to_u8(v):
    """np.uint8 of a float array on x86-64: truncation toward zero, then the low 8 bits."""
    return (np.trunc(np.asarray(v, np.float64)).astype(np.int64) & 255).astype(np.uint8)


def warp_pair(edit_i, edit_next, fwd, bwd, return_float=False):
    """edit frames [H,W,3] (uint8 or 0..255 float), fwd / bwd flows [H,W,2] -> (warped u8, target u8) [H,W,3].
    return_float: also the float32 warped frame before the cast and the mask's (lhs, rhs)."""
    m, lhs, rhs = consistency_mask(fwd, bwd, return_sides=True)
    wf = remap(np.asarray(edit_i, F32), bwd)
    wf = np.where(m[..., None], wf, F32(0))
    tg = np.where(m[..., None], np.asarray(edit_next, F32), F32(0))
    out = (to_u8(wf), to_u8(tg))
    return out + (wf, lhs, rhs) if return_float else out


def _box7(a):
    """sum over every 7x7 window fully inside a [H,W] float64 array -> [H-6, W-6]."""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1))
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim(x, y):
    """x, y uint8 [H,W,3] -> float64 mean SSIM (7x7 uniform window, sample covariance, interior only, mean over channels)."""
    out = []
    n = 49.0
    cov_norm = n / (n - 1)
    for c in range(x.shape[2]):
        X, Y = x[..., c].astype(np.float64), y[..., c].astype(np.float64)
        ux, uy = _box7(X) / n, _box7(Y) / n
        uxx, uyy, uxy = _box7(X * X) / n, _box7(Y * Y) / n, _box7(X * Y) / n
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        out.append(S.mean(dtype=np.float64))
    return float(np.mean(out))


def warp_ssim_from_flows(edit, fut, past):
    """edit [N,H,W,3] u8, fut / past [N,2,H,W] (the flow estimator's layout) -> (mean over pairs, per-pair list).
    Pair i: fwd = fut[i], bwd = past[i + 1]."""
    per = []
    for i in range(len(edit) - 1):
        fwd = np.asarray(fut[i], F32).transpose(1, 2, 0)
        bwd = np.asarray(past[i + 1], F32).transpose(1, 2, 0)
        w, t = warp_pair(edit[i], edit[i + 1], fwd, bwd)
        per.append(ssim(w, t))
    return float(np.mean(per)), per
