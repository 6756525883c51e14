"""Restatements for the tests of the animated light (generation.light_path): the keyframe interpolation, the angle reduction and the unit vectors in
plain Python f64, and tcl_light_ramp_angle_f32's per-pixel sequence in numpy f64 (every operation an array operation of its own: numpy contracts
nothing), written from the header's comment.  TEST INFRASTRUCTURE: nothing here imports the engine."""
import math

import numpy as np

SIZES = ((1, 1), (1, 7), (5, 1), (17, 33), (24, 40))      # (H, W): H*W % 4 != 0 takes the scalar path, (24, 40) the 16 B path
LEVELS = ((255, 0), (224, 32))                             # (hi, lo): tcl_light_gradient_f32's and the bg_source ramps'
ANGLES = (37.5, 135.0, 200.25, 359.999, -45.0, 750.0)      # the last two are reduced to 315 and 30
AXIS = {0.0: ("x", True), 90.0: ("y", True), 180.0: ("x", False), 270.0: ("y", False)}      # reduced angle -> (axis, hi at index 0)


def angles(path, positions):
    """Linear in the angle between the keyframes around each position; keyframes that share a position: the later one holds from there on."""
    out = []
    for p in positions:
        k = max(i for i, (q, _) in enumerate(path) if q <= p)
        if k == len(path) - 1:
            out.append(float(path[k][1]))
        else:
            (p0, a0), (p1, a1) = path[k], path[k + 1]
            out.append(a0 + (a1 - a0) * ((p - p0) / (p1 - p0)))
    return out


def positions(n):
    return [i / (n - 1) if n > 1 else 0.0 for i in range(n)]


def reduce(a):
    r = math.fmod(a, 360.0)
    if r < 0.0:
        r += 360.0
    return 0.0 if r >= 360.0 or r == 0.0 else r


def dirs(angle_list):
    """(c, s) per angle: exactly (1,0) (0,1) (-1,0) (0,-1) at 0 / 90 / 180 / 270, else (cos, sin) of math.radians of the reduced angle."""
    exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    out = []
    for a in angle_list:
        r = reduce(a)
        out.append(exact[r] if r in exact else (math.cos(math.radians(r)), math.sin(math.radians(r))))
    return out


def ramp_d(c, s, H, W):
    """d = px*c + py*s [H,W] f64 and R, as the kernel forms them."""
    c, s = np.float64(c), np.float64(s)
    px = np.arange(W, dtype=np.float64)[None, :] - np.float64(W - 1) / np.float64(2)
    py = np.arange(H, dtype=np.float64)[:, None] - np.float64(H - 1) / np.float64(2)
    a = px * c
    b = py * s
    d = a + b
    R = (np.abs(c) * np.float64(W - 1) + np.abs(s) * np.float64(H - 1)) / np.float64(2)
    return d, R


def ramp_u8(c, s, H, W, hi, lo):
    """[H,W] uint8: t = (R - d)/(2R); when R == 0, t = ((|c| + |s|) + (c + s)) / (2(|c| + |s|)) on every pixel; v = lo + (hi - lo)*t;
    u = trunc(clamp(v, 0, 255))."""
    d, R = ramp_d(c, s, H, W)
    if R == 0:
        c, s = np.float64(c), np.float64(s)
        A = np.abs(c) + np.abs(s)
        t = np.full((H, W), (A + (c + s)) / (np.float64(2) * A))
    else:
        num = R - d
        t = num / (np.float64(2) * R)
    w = np.float64(hi - lo) * t
    v = np.float64(lo) + w
    return np.trunc(np.clip(v, 0.0, 255.0)).astype(np.int64).astype(np.uint8)


def ramp_image(c, s, H, W, hi, lo):
    """[3,H,W] f32 = u/254 (one f32 division), the same plane three times."""
    u = ramp_u8(c, s, H, W, hi, lo)
    return np.broadcast_to(u.astype(np.float32) / np.float32(254), (3, H, W)).copy()


def linspace_u8(reduced, H, W, hi, lo):
    """[H,W] uint8(np.linspace(...)) of the existing ramps for a reduced angle of 0 / 90 / 180 / 270: hi at index 0 for left / top, lo for right /
    bottom, along x for left / right and along y for top / bottom."""
    axis, hi_first = AXIS[reduced]
    a, b = (hi, lo) if hi_first else (lo, hi)
    if axis == "x":
        return np.tile(np.linspace(a, b, W), (H, 1)).astype(np.uint8)
    return np.tile(np.linspace(a, b, H)[:, None], (1, W)).astype(np.uint8)
