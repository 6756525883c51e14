"""Restatement of light-follow (evaluate.py --light; include/tclight_hip.h, "light-follow") in numpy float64, written from the header's definition:
the ten sums, the 3x3 solve, the angle and the two figures -- and, for every sum, the bound that tcl_light_fit_u8's stated float sequence and
summation order allow.  TEST INFRASTRUCTURE: nothing here imports the engine.

What is f32 in the DEFINITION is f32 here too: Ye and Ys (products, sums and the division each one numpy f32 array operation: numpy contracts
nothing), because the clipping weight w is decided on them and must be the same pixel for pixel.  Everything after that is f64.

The bound of a sum (sums_ref returns it as voxel_refs.unproject_ref returns its own: the magnitude the rounding error scales with, times the factor):
with eps = 2^-24, the kernel's
  u = fl(float(2x+1-W) * fl(1/float(W)))                    two conversions, a division, a product: relative error <= 4 eps (v likewise)
  a = fl(Ye + fl(1/255)), b likewise, q = fl(a / b)         (1 + 1) + (1 + 1) + 1 = 5 eps relative, so log q is off by <= 5 eps absolute
  r = logf(q)                                               <= 3 ulp (the OpenCL bound the device library is built to) <= 6 eps |r|
so |r~ - r| <= 6 eps (1 + |r|), and the ten terms are off by at most 13 eps times
  m = (1, |u|, |v|, u^2, |uv|, v^2, 1 + |r|, (1 + |r|)|u|, (1 + |r|)|v|, (1 + |r|)^2)              (worst: rr, 2 * 6 + 1 = 13)
A thread adds 64 terms in f32 (63 additions, <= 63 eps Sum|term| <= 63 eps Sum m); from there on everything is f64: 6 butterfly levels, 3 additions
over the waves, nb over the blocks.  Hence  |sum~ - sum| <= Sum(w m) * (gamma32(77) + gamma64(9 + nb)),  gamma(n) = n e / (1 - n e);  77 = 13 + 63
and one to cover the second-order terms.  Sum w is a sum of at most 2^31 ones: exact, bound 0."""
import math

import numpy as np

SPAN = 16384                       # pixels per block: 4 iterations x 256 threads x 16 pixels
F32_STEPS, F64_FIXED = 77, 9
ANGLES = (0.0, 37.0, 90.0, 200.0, 315.0)
AMPLITUDE = 0.3                    # |g| of the planted plane: see planted()
SIDE_ANGLE = {"left": 0.0, "top": 90.0, "right": 180.0, "bottom": 270.0}


def luma_f32(img):
    """[N,3,H,W] uint8 -> Y f32 [N,H,W] = ((0.299 R + 0.587 G) + 0.114 B) / 255, every operation one f32 array operation."""
    r, g, b = (img[:, k].astype(np.float32) for k in range(3))
    pr, pg, pb = np.float32(0.299) * r, np.float32(0.587) * g, np.float32(0.114) * b
    s = pr + pg
    s = s + pb
    return s / np.float32(255)


def gamma(n, e):
    return n * e / (1 - n * e)


def n_blocks(H, W):
    return (H * W + SPAN - 1) // SPAN


def sums_ref(E, S):
    """E, S uint8 [N,3,H,W] -> (sums f64 [N,10], bound f64 [N,10]) in the order (w, wu, wv, wuu, wuv, wvv, wr, wru, wrv, wrr)."""
    E, S = np.asarray(E), np.asarray(S)
    assert E.dtype == np.uint8 and S.dtype == np.uint8 and E.shape == S.shape and E.ndim == 4 and E.shape[1] == 3
    N, _, H, W = E.shape
    ye, ys = luma_f32(E), luma_f32(S)
    lo, hi = np.float32(2) / np.float32(255), np.float32(253) / np.float32(255)
    w = ((ye >= lo) & (ye <= hi) & (ys >= lo) & (ys <= hi)).astype(np.float64)
    c = 1.0 / 255.0
    r = np.log((ye.astype(np.float64) + c) / (ys.astype(np.float64) + c))
    u = np.broadcast_to(((2.0 * np.arange(W) + 1.0) / W - 1.0)[None, None, :], (N, H, W))
    v = np.broadcast_to(((2.0 * np.arange(H) + 1.0) / H - 1.0)[None, :, None], (N, H, W))
    one = np.ones_like(w)
    terms = (one, u, v, u * u, u * v, v * v, r, r * u, r * v, r * r)
    ar = 1.0 + np.abs(r)
    mags = (one, np.abs(u), np.abs(v), u * u, np.abs(u * v), v * v, ar, ar * np.abs(u), ar * np.abs(v), ar * ar)
    sums = np.stack([(w * t).sum(axis=(1, 2)) for t in terms], axis=1)
    factor = gamma(F32_STEPS, 2.0 ** -24) + gamma(F64_FIXED + n_blocks(H, W), 2.0 ** -53)
    bound = np.stack([(w * m).sum(axis=(1, 2)) for m in mags], axis=1) * factor
    bound[:, 0] = 0.0
    return sums, bound


def solve_ref(row):
    """One frame's ten sums -> (estimate?, angle in degrees [0, 360), contrast, R^2), by Cramer's rule in f64.  No estimate: Sw < 3, a determinant
    not above 1e-12 Sw Swuu Swvv (singular), or contrast 0."""
    sw, swu, swv, swuu, swuv, swvv, swr, swru, swrv, swrr = (float(x) for x in row)
    if not sw >= 3.0:
        return False, None, None, None

    def det3(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    A = [[sw, swu, swv], [swu, swuu, swuv], [swv, swuv, swvv]]
    b = [swr, swru, swrv]
    d = det3(A)
    if not d > 1e-12 * sw * swuu * swvv:
        return False, None, None, None
    x = []
    for k in range(3):
        M = [[b[i] if j == k else A[i][j] for j in range(3)] for i in range(3)]
        x.append(det3(M) / d)
    a, gx, gy = x
    contrast = math.hypot(gx, gy)
    if not contrast > 0.0:
        return False, None, None, None
    angle = math.degrees(math.atan2(-gy, -gx)) % 360.0
    ss_res = swrr - (a * swr + gx * swru + gy * swrv)
    ss_tot = swrr - swr * swr / sw
    return True, angle, contrast, (1.0 - ss_res / ss_tot if ss_tot > 0.0 else 0.0)


def figures_ref(sums, wanted):
    """-> (light-follow, light-contrast): the means over the frames of cos(angle - wanted) and of the contrast; a frame without an estimate counts 0."""
    cs, ks = [], []
    for row, want in zip(sums, wanted):
        ok, ang, con, _ = solve_ref(row)
        cs.append(math.cos(math.radians(ang - want)) if ok else 0.0)
        ks.append(con if ok else 0.0)
    return float(np.mean(cs)), float(np.mean(ks))


def angle_diff(a, b):
    """|a - b| on the circle, degrees."""
    return abs((a - b + 180.0) % 360.0 - 180.0)


def angle_bound_deg(row, bound):
    """The angle error (degrees) that per-sum errors of at most `bound` allow in the fit of `row`: with A x = b the normal equations,
    |dx| <= |A^-1| (|dA| |x| + |db|) / (1 - rho), rho = || |A^-1| |dA| ||_inf  (the standard componentwise perturbation bound), and a gradient
    moved by at most hypot(dgx, dgy) turns by at most asin of that over its length."""
    s, e = [float(x) for x in row], [float(x) for x in bound]
    A = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    dA = np.array([[e[0], e[1], e[2]], [e[1], e[3], e[4]], [e[2], e[4], e[5]]])
    b, db = np.array(s[6:9]), np.array(e[6:9])
    Ai = np.abs(np.linalg.inv(A))
    x = np.linalg.solve(A, b)
    rho = float((Ai @ dA).sum(axis=1).max())
    assert rho < 0.5
    dx = Ai @ (dA @ np.abs(x) + db) / (1.0 - rho)
    q = math.hypot(dx[1], dx[2]) / math.hypot(x[1], x[2])
    assert q < 1.0
    return math.degrees(math.asin(q))


def planted(N, H, W, angles, seed, amplitude=AMPLITUDE, a=0.0):
    """(E, S) uint8 [N,3,H,W]: S random mid-grey (64..160, R = G = B), E = round(S exp(a + gx u + gy v)) with (gx, gy) = -amplitude (cos, sin) of
    the frame's angle, so the light comes FROM that angle.  amplitude 0.3: E stays below 160 exp(0.3 sqrt 2) = 245 < 253 (nothing clips), and the
    rounding of E (0.5 / 64 relative at worst, over ~2000 pixels) moves the fitted gradient by ~1e-3 of its length -- far inside the 2 degrees
    the CPU test asks of the inputs."""
    rng = np.random.default_rng(seed)
    g = rng.integers(64, 161, (N, 1, H, W))
    u = ((2.0 * np.arange(W) + 1.0) / W - 1.0)[None, None, None, :]
    v = ((2.0 * np.arange(H) + 1.0) / H - 1.0)[None, None, :, None]
    th = np.radians(np.asarray(angles, dtype=np.float64))[:, None, None, None]
    e = np.rint(g * np.exp(a - amplitude * np.cos(th) * u - amplitude * np.sin(th) * v))
    S = np.broadcast_to(g, (N, 3, H, W)).astype(np.uint8)
    E = np.broadcast_to(np.clip(e, 0, 255), (N, 3, H, W)).astype(np.uint8)
    return np.ascontiguousarray(E), np.ascontiguousarray(S)
