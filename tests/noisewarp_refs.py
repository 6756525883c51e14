"""numpy reference of generation.noise_mode warp: the chain of include/tclight_hip.h (section "flow-warped noise") in the kernel's own f32 / integer
sequence (chain), the same in float64 with the exact mean in place of the fixed-point one (f64=True, with a per-element error bound of the f32
sequence), and the naive transport without the conditional term (naive=True: a valid pixel copies its source whatever k is) -- what the statistics
tests show to be wrong.  Also the flow cases of the GPU tests and the statistics the CPU tests bound."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
CELL = 8
FIX = 16777216.0                 # 2^24: the fixed-point scale of the sums
U = 2.0 ** -24                   # unit roundoff of f32


def source_map(flow, mask):
    """flow [2,H,W] f32, mask [H,W] f32 -> q int64 [H,W]: the offset qy * W + qx of every valid pixel's source, -1 where the pixel is invalid.
    f32 throughout, np.rint rounds ties to even as rintf does; every comparison with a NaN is false."""
    _, H, W = flow.shape
    x = np.arange(W, dtype=F32)[None, :]
    y = np.arange(H, dtype=F32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        qx = np.rint(x + flow[0].astype(F32))
        qy = np.rint(y + flow[1].astype(F32))
        valid = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1) & (mask.astype(F32) > F32(0.5))
    qx = np.where(valid, qx, 0).astype(I64)
    qy = np.where(valid, qy, 0).astype(I64)
    return np.where(valid, qy * W + qx, -1)


def count(G, q):
    """G [4,H,W] f32, q of source_map -> (k int32 [H,W], S int64 [4,H,W]): per source, the number of valid pixels that pick it and the sums of
    llrintf(G * 2^24) over them."""
    _, H, W = G.shape
    v = q >= 0
    k = np.bincount(q[v], minlength=H * W).astype(np.int32)
    fix = np.rint(G.astype(F32) * F32(FIX)).astype(I64)             # G * 2^24 is exact in f32; rint of an f32 is an f32
    S = np.zeros((4, H * W), dtype=I64)
    for c in range(4):
        np.add.at(S[c], q[v], fix[c][v])
    return k.reshape(H, W), S.reshape(4, H, W)


def step(G, Fp, q, k, S, f64=False, naive=False, Ep=None):
    """One frame t >= 1 -> F [4,H,W] (f32, or f64 with f64=True; then also E, the bound of |F_f32 - F_f64| per element given Ep of the frame before)."""
    _, H, W = G.shape
    T = F64 if f64 else F32
    Gt = G.astype(T)
    F = Gt.copy().reshape(4, -1)
    E = np.zeros((4, H * W)) if f64 else None
    qf, kf = q.reshape(-1), k.reshape(-1)
    v = qf >= 0
    kq = np.where(v, kf[np.where(v, qf, 0)], 0)
    one = v & ((kq == 1) | naive)
    many = v & (kq > 1) & (not naive)
    Fp = Fp.reshape(4, -1)
    F[:, one] = Fp[:, qf[one]]
    if f64 and Ep is not None:
        E[:, one] = Ep.reshape(4, -1)[:, qf[one]]
    if many.any():
        qm, km = qf[many], kq[many]
        if f64:                                                     # the exact mean of G over the pixels that share the source
            Sx = np.zeros((4, H * W))
            for c in range(4):
                np.add.at(Sx[c], qf[v], Gt.reshape(4, -1)[c][v])
            mean = Sx[:, qm] / km.astype(F64)
            a = Fp[:, qm] / np.sqrt(km.astype(F64))
        else:
            mean = (S.reshape(4, -1)[:, qm].astype(F64) / (FIX * km.astype(F64))).astype(F32)
            a = Fp[:, qm] / np.sqrt(km.astype(F32))
        b = Gt.reshape(4, -1)[:, many] - mean
        F[:, many] = a + b
        if f64:     # the f32 sequence: each G enters the sum with an error of at most 2^-25, then one rounding each of mean, a, b and a + b
            ep = 0.0 if Ep is None else Ep.reshape(4, -1)[:, qm] / np.sqrt(km.astype(F64))
            E[:, many] = ep + 2.0 ** -25 + U * (2 * np.abs(mean) + 2 * np.abs(a) + 2 * np.abs(b) + np.abs(a + b))
    return (F.reshape(4, H, W), E.reshape(4, H, W)) if f64 else F.reshape(4, H, W)


def reduce8(F):
    """F [4,H,W] -> z [4,H/8,W/8] in F's dtype: the 8 pixels of a row left to right, the 8 row sums top to bottom, one multiplication by 1/8."""
    c, H, W = F.shape
    x = F.reshape(c, H // CELL, CELL, W // CELL, CELL)
    r = x[..., 0]
    for j in range(1, CELL):
        r = r + x[..., j]
    s = r[:, :, 0]
    for i in range(1, CELL):
        s = s + r[:, :, i]
    return s * F.dtype.type(0.125)


def chain(G, flows, masks, f64=False, naive=False, detail=False):
    """G [N,4,H,W] f32 (the fresh fields), flows [N,2,H,W] f32, masks [N,1,H,W] f32 -> z [N,4,h,w] (f32; f64=True: float64).
    detail: -> (z, [F_t], [k_t], [S_t]) (k, S None for t = 0).  f64 and detail: -> (z, bound [N,4,h,w] of |z_f32 - z_f64|)."""
    N = G.shape[0]
    T = F64 if f64 else F32
    F = G[0].astype(T)
    E = np.zeros(F.shape)
    zs, Fs, ks, Ss, bs = [reduce8(F)], [F], [None], [None], []
    bs.append(_reduce_bound(F, E))
    for t in range(1, N):
        q = source_map(flows[t], masks[t, 0])
        k, S = count(G[t], q)
        if f64:
            F, E = step(G[t], F, q, k, S, f64=True, naive=naive, Ep=E)
        else:
            F = step(G[t], F, q, k, S, naive=naive)
        zs.append(reduce8(F)); Fs.append(F); ks.append(k); Ss.append(S); bs.append(_reduce_bound(F, E))
    z = np.stack(zs)
    if f64 and detail:
        return z, np.stack(bs)
    return (z, Fs, ks, Ss) if detail else z


def _reduce_bound(F, E):
    """|z_f32 - z_f64| per latent sample: the elements' own errors E plus 63 sequential f32 additions and one exact scaling -- the textbook bound
    (n - 1) u sum |x_i| of recursive summation, with n = 64 (and one more u for the first-order terms dropped)."""
    c, H, W = F.shape
    blocks = lambda a: a.reshape(c, H // CELL, CELL, W // CELL, CELL).sum(axis=(2, 4))
    return (blocks(np.abs(E)) + 64 * U * blocks(np.abs(F) + np.abs(E))) / CELL


# ---------------------------------------------------------------------------------------------------------------- flows
def grid(H, W):
    return np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))       # (x [H,W], y [H,W])


def translation(N, H, W, dx, dy):
    """Every frame's content sits (dx, dy) further than the frame before: the backward flow is (-dx, -dy)."""
    f = np.zeros((N, 2, H, W), dtype=F32)
    f[1:, 0], f[1:, 1] = -dx, -dy
    return f


def zoom(N, H, W, s):
    """The content grows by the factor s about the centre per frame: pixel p of frame t shows c + (p - c) / s of frame t-1."""
    x, y = grid(H, W)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    f = np.zeros((N, 2, H, W), dtype=F32)
    f[1:, 0] = ((x - cx) / s - (x - cx)).astype(F32)
    f[1:, 1] = ((y - cy) / s - (y - cy)).astype(F32)
    return f


def one_source(N, H, W):
    """Every pixel of every frame has the same source: k = H * W there."""
    x, y = grid(H, W)
    f = np.zeros((N, 2, H, W), dtype=F32)
    f[1:, 0], f[1:, 1] = (W // 3 - x).astype(F32), (H // 2 - y).astype(F32)
    return f


def nonfinite(N, H, W, seed=3):
    """A rough flow of a few pixels with NaN, +-inf, huge and just-out-of-frame targets sprinkled over it."""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((N, 2, H, W)) * 3).astype(F32)
    bad = np.array([np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1.0e9, float(W), -float(W), float(H), -float(H), -0.0], dtype=F32)
    hit = rng.random((N, 2, H, W)) < 0.2
    f[hit] = bad[rng.integers(0, len(bad), int(hit.sum()))]
    f[0] = 0
    return f


def edge_masks(N, H, W, seed=4):
    """Masks exactly at 0.5, one ulp either side of it, 0, 1, and a NaN."""
    rng = np.random.default_rng(seed)
    vals = np.array([0.5, np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0)), 0.0, 1.0, 0.75, np.nan], dtype=F32)
    return vals[rng.integers(0, len(vals), (N, 1, H, W))]


def ones(N, H, W):
    return np.ones((N, 1, H, W), dtype=F32)


def cases(N, H, W):
    """name -> (flows [N,2,H,W], masks [N,1,H,W]): what the GPU tests compare bit for bit."""
    rng = np.random.default_rng(11)
    soft = (0.5 + 0.6 * rng.standard_normal((N, 1, H, W))).astype(F32)
    return {
        "zero": (translation(N, H, W, 0, 0), ones(N, H, W)),
        "integer": (translation(N, H, W, 5, -3), ones(N, H, W)),
        "half": (translation(N, H, W, -2.5, 0.5), ones(N, H, W)),                 # x + 2.5, y - 0.5: every target is a tie
        "zoom_in": (zoom(N, H, W, 2.0), soft),
        "zoom_out": (zoom(N, H, W, 0.5), ones(N, H, W)),
        "one_source": (one_source(N, H, W), ones(N, H, W)),
        "nonfinite": (nonfinite(N, H, W), soft),
        "mask_edge": (translation(N, H, W, 1, 1) + (rng.standard_normal((N, 2, H, W)) * 0.7).astype(F32) * (np.arange(N) > 0)[:, None, None, None],
                      edge_masks(N, H, W)),
    }


def fields(N, H, W, seed=0):
    return np.random.default_rng(seed).standard_normal((N, 4, H, W)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- statistics
def stats(z):
    """z [4,h,w] -> (mean, variance, horizontal and vertical neighbour covariance) in float64."""
    z = z.astype(F64)
    return (float(z.mean()), float(z.var()), float((z[:, :, 1:] * z[:, :, :-1]).mean()), float((z[:, 1:] * z[:, :-1]).mean()))


def bounds(n):
    """For n independent unit-variance samples: 5 standard deviations of the sample mean / covariance (1 / sqrt(n)) and of the sample variance
    (sqrt(2 / n)) -> (mean and covariance bound, variance bound)."""
    return 5.0 / np.sqrt(n), 5.0 * np.sqrt(2.0 / n)


def white(z):
    """Is z [4,h,w] inside the bounds of white unit-variance noise?"""
    m, v, ch, cv = stats(z)
    bm, bv = bounds(z.size)
    return abs(m) <= bm and abs(v - 1.0) <= bv and abs(ch) <= bm and abs(cv) <= bm
