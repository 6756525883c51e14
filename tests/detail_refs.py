"""Float64 reference, case table and error bound of generation.detail_transfer (tcl_detail_transfer_f32, csrc/detail.hip).

The maths (S source, R relit, m weight or 1, b strength, all per frame):
  G         separable Gaussian, radius r = ceil(3 sigma), taps w_k = exp(-k^2 / 2 sigma^2) / sum in float64 rounded once to f32 (detail.gaussian_taps --
            the reference uses those f32 values, so the taps carry no error), borders reflected without repeating the edge sample.
  Y(x)      0.299 x_R + 0.587 x_G + 0.114 x_B
  add       D = S - R;  P = D - G(D)  (luma: P = Y(D) - G(Y(D)), one P for the three channels);  O = clamp(R + b m P, 0, 1)
  ratio     T = S (G(R) + e) / (G(S) + e), e = 1/255  (luma: the ratio of G(Y(R)) and G(Y(S)));  O = clamp(R + b m (T - R), 0, 1)

The bound, per element, from the arithmetic alone (u = 2^-24, the unit roundoff of f32; gamma(k) = k u / (1 - k u), Higham's constant):
  * a sum of n = 2r + 1 products with one rounding per term (an fma chain, any order) is off by at most gamma(n) * sum w_k |v_k|; the taps are
    non-negative, so sum w_k |v_k| = G(|v|).  Two passes, the second on the first's rounded result, inputs v themselves off by a relative g_in:
        |G_f32(v) - G(v)|  <=  ((1 + gamma(n))^2 (1 + g_in) - 1) * G(|v|)  =: E_G.
    g_in: u for D = fl(S - R); for a luminance three more operations and three rounded coefficients on top, gamma(6) of Y(|x|) (>= |Y(x)|); the
    inputs R, S of `ratio` are exact.
  * add:  P = fl(v - G_f32):  |dP| <= g_in |v| + E_G + u |P|.
  * ratio:  num = fl(G_f32(R) + e32), den likewise (e32 = fl(1/255): relative u):  rel(num) <= (E_G(R) + u e) / (G(R) + e) + u, the same for den;
    q = fl(num / den), T = fl(S q):  |dT| <= |T| * ((1 + rel(num)) (1 + u)^2 / (1 - rel(den)) - 1), and |T| = S / (G(S) + e) * (G(R) + e): the bound
    scales with the float64 value of S / (G(S) + e) at the element.  Then d = fl(T - R): u |d| more.
  * the blend, with X = P or T - R:  bm = fl(b m), t = fl(bm X), o = fl(R + t):  |dO| <= bm |dX| (1 + u)^3 + ((1 + u)^3 - 1) |bm X| + u |R + bm X|.
    The clamp is exact and 1-Lipschitz.
Nothing in it is tuned; at these sizes it is a few 1e-7 for add and up to a few 1e-5 for ratio where S / (G(S) + e) is large.
"""
import math

import numpy as np

U = 2.0 ** -24
EPS = 1.0 / 255.0
LUMA_W = (0.299, 0.587, 0.114)


def gamma(k):
    return k * U / (1.0 - k * U)


def taps_f32(sigma):
    """What detail.gaussian_taps computes, restated: (f32 taps, r)."""
    r = int(math.ceil(3.0 * float(sigma)))
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).astype(np.float32), r


def reflect_index(L, r):
    """Source index of every position -r .. L-1+r: -i -> i, L-1+i -> L-1-i."""
    i = np.abs(np.arange(-r, L + r))
    return np.where(i > L - 1, 2 * (L - 1) - i, i)


def repeat_index(L, r):
    """The planted defect: the symmetric border that repeats the edge sample (-1 -> 0, L -> L-1)."""
    i = np.arange(-r, L + r)
    i = np.where(i < 0, -i - 1, i)
    return np.where(i > L - 1, 2 * L - 1 - i, i)


def blur(x, taps, index=reflect_index):
    """x [..., H, W] float64, taps [2r + 1] (any float dtype) -> G(x), rows first, then columns, in float64."""
    w = np.asarray(taps, dtype=np.float64)
    r = (len(w) - 1) // 2
    H, W = x.shape[-2:]
    xp = x[..., index(W, r)]
    h = sum(w[k] * xp[..., k:k + W] for k in range(2 * r + 1))
    hp = h[..., index(H, r), :]
    return sum(w[k] * hp[..., k:k + H, :] for k in range(2 * r + 1))


def luma(x):
    """x [N,3,H,W] -> [N,1,H,W]"""
    return (LUMA_W[0] * x[:, 0] + LUMA_W[1] * x[:, 1] + LUMA_W[2] * x[:, 2])[:, None]


def reference(S, R, mask, sigma, mode, channels, blend):
    """S, R [N,3,H,W] f32, mask [N,1,H,W] f32 or None -> (O float64, per-element bound float64)."""
    taps, r = taps_f32(sigma)
    n = 2 * r + 1
    S, R = S.astype(np.float64), R.astype(np.float64)
    bm = float(np.float32(blend)) * (np.ones_like(S[:, :1]) if mask is None else mask.astype(np.float64))
    lum = channels == "luma"
    if mode == "add":
        D = S - R
        v, absv, g_in = (luma(D), luma(np.abs(D)), (1 + U) * (1 + gamma(6)) - 1) if lum else (D, np.abs(D), U)
        Gv = blur(v, taps)
        E_G = ((1 + gamma(n)) ** 2 * (1 + g_in) - 1) * blur(absv, taps)
        X = v - Gv
        dX = g_in * absv + E_G
        dX = dX + U * (np.abs(X) + dX)
    else:
        g_in = gamma(6) if lum else 0.0
        a, b = (luma(R), luma(S)) if lum else (R, S)
        GR, GS = blur(a, taps), blur(b, taps)
        c = (1 + gamma(n)) ** 2 * (1 + g_in) - 1
        rel_n, rel_d = (c * GR + U * EPS) / (GR + EPS) + U, (c * GS + U * EPS) / (GS + EPS) + U
        T = S / (GS + EPS) * (GR + EPS)
        dT = np.abs(T) * ((1 + rel_n) * (1 + U) ** 2 / (1 - rel_d) - 1)
        X = T - R
        dX = dT + U * (np.abs(X) + dT)
    O = R + bm * X
    dO = bm * dX * (1 + U) ** 3 + ((1 + U) ** 3 - 1) * np.abs(bm * X) + U * (np.abs(O) + bm * dX)
    return np.clip(O, 0.0, 1.0), dO


# ---------------------------------------------------------------------------------------------------------------- f32 emulation of the kernel
def _fma_chain(xp, taps, n_out, axis):
    """a = 0; a = fl32(a + w_k v_k) for k ascending (the product of two f32 is exact in f64; the sum is rounded to f64, then f32)."""
    acc = np.zeros(tuple(n_out if d == axis % xp.ndim else s for d, s in enumerate(xp.shape)), dtype=np.float32)
    for k in range(len(taps)):
        sl = [slice(None)] * xp.ndim
        sl[axis] = slice(k, k + n_out)
        acc = (acc.astype(np.float64) + np.float64(taps[k]) * xp[tuple(sl)].astype(np.float64)).astype(np.float32)
    return acc


def blur_f32(x, taps, index=reflect_index):
    r = (len(taps) - 1) // 2
    H, W = x.shape[-2:]
    h = _fma_chain(x[..., index(W, r)], taps, W, -1)
    return _fma_chain(h[..., index(H, r), :], taps, H, -2)


def _luma_f32(x):
    f = np.float32
    a = f(0.299) * x[:, 0]
    b = (np.float64(f(0.587)) * x[:, 1].astype(np.float64) + a.astype(np.float64)).astype(f)
    return (np.float64(f(0.114)) * x[:, 2].astype(np.float64) + b.astype(np.float64)).astype(f)[:, None]


def emulate_f32(S, R, mask, sigma, mode, channels, blend, taps=None, index=reflect_index, use_mask=True):
    """The kernel's operation sequence in numpy f32 (include/tclight_hip.h).  taps / index / use_mask plant the defects of the CPU tests."""
    f = np.float32
    if taps is None:
        taps, _ = taps_f32(sigma)
    taps = np.asarray(taps, dtype=f)
    S, R = S.astype(f), R.astype(f)
    bm = f(blend) * mask.astype(f) if (mask is not None and use_mask) else f(blend)
    lum = channels == "luma"
    if mode == "add":
        D = S - R
        v = _luma_f32(D) if lum else D
        X = v - blur_f32(v, taps, index)
    else:
        a, b = (_luma_f32(R), _luma_f32(S)) if lum else (R, S)
        num, den = blur_f32(a, taps, index) + f(1.0) / f(255.0), blur_f32(b, taps, index) + f(1.0) / f(255.0)
        X = S * (num / den) - R
    t = (bm * X).astype(f)
    return np.clip((R + t).astype(f), f(0), f(1))


# ---------------------------------------------------------------------------------------------------------------- cases
def tile_sizes():
    """(row segment, tile width, tile height) of the kernels, as tc_light_amd/detail.py reads them from the header."""
    from tc_light_amd import detail
    return detail.ROW_SEG, detail.TILE_W, detail.TILE_H


def geometries():
    """name -> (N, H, W, sigma, masked)."""
    seg, tw, th = tile_sizes()
    g = {"overlap_3x5": (2, 3, 5, 0.5, True),                   # r = 2 = min(H, W) - 1: the reflections from both borders overlap
         "overlap_4x7": (2, 4, 7, 1.0, False),                  # r = 3
         "rmax_49x130": (1, 49, 130, 16.0, True)}               # r = 48 at the smallest legal height, more than one tile across
    for d in (-1, 0, 1):
        g[f"tile{d:+d}"] = (2, th + d, tw + d, 2.0, d == 0)     # r = 6
        g[f"seg{d:+d}"] = (1, 9, seg + d, 1.5, d != 0)          # r = 5
    return g


SETTINGS = [("add", "rgb"), ("add", "luma"), ("ratio", "rgb"), ("ratio", "luma")]
BLEND = 0.75                                                    # exact in f32; 1.0 is covered by the identity tests

_MADE = {}


def inputs(name):
    """Seeded S, R (and mask) of one geometry, made once: S textured, R a re-lit, softened S (different per frame), both f32 in [0,1] with exact 0s
    and 1s; the mask holds 0, 1 and fractions."""
    if name not in _MADE:
        N, H, W, sigma, masked = geometries()[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        S = rng.random((N, 3, H, W))
        S[rng.random(S.shape) < 0.05] = 0.0
        S[rng.random(S.shape) < 0.05] = 1.0
        ramp = np.linspace(0.3, 1.2, W)[None, None, None, :] * np.linspace(1.1, 0.6, N)[:, None, None, None]
        R = np.clip(0.6 * S * ramp + 0.4 * S.mean(axis=(2, 3), keepdims=True) * ramp + 0.02 * rng.standard_normal(S.shape), 0.0, 1.0)
        mask = None
        if masked:
            mask = rng.random((N, 1, H, W))
            mask[rng.random(mask.shape) < 0.3] = 0.0
            mask[rng.random(mask.shape) < 0.3] = 1.0
            mask = mask.astype(np.float32)
        _MADE[name] = (S.astype(np.float32), R.astype(np.float32), mask, sigma)
    return _MADE[name]


_REFS = {}


def case(name, mode, channels):
    """-> dict(S, R, mask, sigma, ref, bound) of one (geometry, setting): computed once, shared, left unchanged."""
    key = (name, mode, channels)
    if key not in _REFS:
        S, R, mask, sigma = inputs(name)
        ref, bound = reference(S, R, mask, sigma, mode, channels, BLEND)
        _REFS[key] = dict(S=S, R=R, mask=mask, sigma=sigma, ref=ref, bound=bound)
    return _REFS[key]
