"""Float64 restatements of tcl_flow_chain_f32 and tcl_keyframe_propagate_f32, written from the text at their prototypes in include/tclight_hip.h (not
from the kernels), the per-element error bound of an f32 implementation in the stated operation order, and the case table of the keyframe tests.

What is restated in float32 on purpose: q = p + A in the chain has exact f32 inputs and ONE rounding, so the kernel's q is np.float32(x) + A bit
for bit; the reference takes that value, and inb(q), floor(q) and the fractions of the chain are then the kernel's exactly.  Everything behind it is
float64.

The bound (U = 2^-24, one f32 rounding; M = the largest |tap| of a bil):
  bil            3 lerps a + f (b - a), each  <= 2U f |b - a| + U |result| <= 5 U M;  two levels: 10 U M            (fractions exact: q - floor(q))
  chain          E_1 = 0 (C = A);  E_d(p) = max over the taps of E_{d-1} + 10 U M + U |C|                            (no position error: q is exact)
  propagate      q = p + C has the position error e_q = E + U |q|; a bil at q moves by at most Lx e_qx + Ly e_qy, L the largest tap difference
                 of the 2 x 2 cell and its neighbours (bil is continuous and piecewise bilinear, so this holds across a changed floor too):
                 e_s = L . e_q + 10 U M (and e_r);  n = r + eps, d = s + eps: e_n = e_r + U |n|;  G = n / d: e_G = (e_n + |G| e_d) / (d - e_d) + U |G|;
                 blend (w_a G_a + w_b G_b) / w: (w_a e_Ga + w_b e_Gb) / w + 5 U (w_a |G_a| + w_b |G_b|) / w  (two products, a sum, the sum w, a
                 division); hole ta G'_a + tb G'_b: 6 U (ta |G'_a| + tb |G'_b|) (three roundings in each G', two products, a sum);
                 out = (S + eps) G - eps: |S + eps| e_G + 2 U |S + eps| |G| + U |out|
  The test bound is SAFETY = 2 times this first-order sum (the neglected products of two errors are below U times it) plus 1e-12.
A threshold comparison can fall differently in f32: a pixel whose float64 margin at a gate is below DELTA -- | sqrt(lhs) - t | for fb, | m - diff_threshold |
for photo (inb is exact, see above; w_a + w_b > 0 is decided by the other gates) -- is ambiguous and left out, as is every chain pixel one of whose four
taps is, and every output pixel whose CL or CR is.  DELTA = 1e-3 (pixels / intensity) is far above the f32 error of either side (below 1e-4 here)."""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
DELTA = 1e-3
MAX_AMBIGUOUS = 0.02
ALPHA, DIFF, EPS = 0.1, 0.1, 1.0 / 64
TILE_W, TILE_H = 64, 4               # TCL_KEYFRAME_TILE_W / _H (tests/test_gpu_keyframe.py checks them against the header)

# name -> (N, K, H, W, family)
CASES = {
    "n9k4_37x70_integer": (9, 4, 37, 70, "integer"), "n9k4_37x70_lattice": (9, 4, 37, 70, "lattice"), "n9k4_37x70_smooth": (9, 4, 37, 70, "smooth"),
    "n6k4_33x129_integer": (6, 4, 33, 129, "integer"), "n6k4_33x129_smooth": (6, 4, 33, 129, "smooth"),
    "n2k16_tile_lattice": (2, 16, TILE_H, TILE_W, "lattice"), "n5k2_tile+1_integer": (5, 2, TILE_H + 1, TILE_W + 1, "integer"),
    "n5k2_tile+1_smooth": (5, 2, TILE_H + 1, TILE_W + 1, "smooth"), "n5k2_37x70_lattice": (5, 2, 37, 70, "lattice"),
    "n17k16_37x70_integer": (17, 16, 37, 70, "integer"), "n17k16_33x129_smooth": (17, 16, 33, 129, "smooth"),
    "n17k16_33x129_lattice": (17, 16, 33, 129, "lattice"),
}


def keyframe_ids(n, k):
    ids = list(range(0, n, k))
    return ids if ids[-1] == n - 1 else ids + [n - 1]


def tables(keys, n):
    """left / right key INDEX of every frame and the weights [2, n] f32 (float64, rounded once), as the header states them."""
    k = np.asarray(keys)
    left = np.array([int(np.nonzero(k <= i)[0][-1]) for i in range(n)])
    right = np.array([int(np.nonzero(k >= i)[0][0]) for i in range(n)])
    ta = np.array([1.0 if left[i] == right[i] else (k[right[i]] - i) / (k[right[i]] - k[left[i]]) for i in range(n)], dtype=np.float64)
    return left, right, np.stack([ta, 1.0 - ta]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ bil
def _cell(qx, qy, H, W):
    qx, qy = np.clip(qx, 0.0, W - 1.0), np.clip(qy, 0.0, H - 1.0)
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    return x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1), qx - x0.astype(qx.dtype), qy - y0.astype(qy.dtype)


def taps(T, qx, qy):
    """T [..., H, W] -> the four taps (t00, t01, t10, t11) at q and the fractions."""
    H, W = T.shape[-2:]
    x0, x1, y0, y1, fx, fy = _cell(qx, qy, H, W)
    return (T[..., y0, x0], T[..., y0, x1], T[..., y1, x0], T[..., y1, x1]), fx, fy


def bil(T, qx, qy, dt=np.float64):
    (a, b, c, d), fx, fy = taps(T.astype(dt), qx, qy)
    fx, fy = fx.astype(dt), fy.astype(dt)
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    return top + fy * (bot - top)


def tap_max(T, qx, qy):
    (a, b, c, d), _, _ = taps(np.abs(T), qx, qy)
    return np.maximum(np.maximum(a, b), np.maximum(c, d))


def lipschitz(T):
    """-> (Lx, Ly) [..., H, W]: at cell origin (y0, x0) the largest |difference of horizontal / vertical neighbours| among the cell and the cells around
    it (a 4 x 4 pixel neighbourhood), so a q that crosses into a neighbouring cell by a rounding is covered."""
    H, W = T.shape[-2:]
    dx = np.zeros_like(T); dx[..., :, :-1] = np.abs(np.diff(T, axis=-1))
    dy = np.zeros_like(T); dy[..., :-1, :] = np.abs(np.diff(T, axis=-2))

    def grow(a):
        p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 2), (1, 2)], mode="edge")
        return np.max([p[..., i:i + H, j:j + W] for i in range(4) for j in range(4)], axis=0)
    return grow(dx), grow(dy)


# ------------------------------------------------------------------------------------------------------------------ the chain
def chain_ref(fut, past, keys, alpha=ALPHA, clamp_instead_of_invalidate=False):
    """-> C [N,2,3,H,W] float64 (direction 0 = CL, 1 = CR; planes dx, dy, valid; zeros at key frames), E [N,2,H,W] the bound of an f32 kernel's error
    on dx / dy, amb [N,2,H,W] the ambiguous pixels.  clamp_instead_of_invalidate: the planted defect -- inb(q) is not part of `valid`."""
    N, _, H, W = fut.shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    C = np.zeros((N, 2, 3, H, W)); E = np.zeros((N, 2, H, W)); amb = np.zeros((N, 2, H, W), dtype=bool)
    for a, b in zip(keys, keys[1:]):
        for d in range(1, b - a):
            for direction, (j, own, back, prev) in enumerate(((a + d, past, fut, a + d - 1), (b - d, fut, past, b - d + 1))):
                A = own[j]                                                  # f32
                qx, qy = (xs + A[0]).astype(np.float64), (ys + A[1]).astype(np.float64)      # the kernel's q, bit for bit
                A = A.astype(np.float64)
                g = bil(back[prev].astype(np.float64), qx, qy)
                lhs = (A[0] + g[0]) ** 2 + (A[1] + g[1]) ** 2
                t = alpha * (np.sqrt(A[0] ** 2 + A[1] ** 2) + np.sqrt(g[0] ** 2 + g[1] ** 2)) + alpha
                inb = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
                valid = (lhs < t * t) & (True if clamp_instead_of_invalidate else inb)
                am = inb & (np.abs(np.sqrt(lhs) - t) < DELTA)
                cx, cy, e = A[0], A[1], np.zeros((H, W))
                if d > 1:
                    P = C[prev, direction]
                    cx, cy = A[0] + bil(P[0], qx, qy), A[1] + bil(P[1], qx, qy)
                    v4, _, _ = taps(P[2], qx, qy)
                    valid &= (v4[0] == 1) & (v4[1] == 1) & (v4[2] == 1) & (v4[3] == 1)
                    a4, _, _ = taps(amb[prev, direction], qx, qy)
                    am |= inb & (a4[0] | a4[1] | a4[2] | a4[3])
                    e4, _, _ = taps(E[prev, direction], qx, qy)
                    e = np.max(e4, axis=0) + 10 * U * tap_max(P[:2], qx, qy).max(axis=0) + U * np.maximum(np.abs(cx), np.abs(cy))
                C[j, direction] = np.stack([np.where(valid, cx, 0.0), np.where(valid, cy, 0.0), valid.astype(np.float64)])
                E[j, direction] = np.where(valid, e, 0.0)
                amb[j, direction] = am
    return C, E, amb


def fb_of_the_reference(fwd, bwd_at_q, alpha=ALPHA):
    """compute_fwdbwd_mask's inequality (utils/flow_utils.py of the reference) on a flow and the opposite flow sampled at its target:
    |fwd + bwd| < alpha (|fwd| + |bwd|) + alpha, norms over the two components."""
    n = lambda v: np.sqrt(v[0] ** 2 + v[1] ** 2)
    return n(fwd + bwd_at_q) < alpha * (n(fwd) + n(bwd_at_q)) + alpha


# ------------------------------------------------------------------------------------------------------------------ the propagation
def propagate_ref(S, R, keys, C, E=None, amb=None, thr=DIFF, eps=EPS, swap_t=False, no_hole_fallback=False, keep_eps=False, dt=np.float64):
    """-> out [N,3,H,W], holes [N], bound [N,3,H,W], left_out [N,H,W] (ambiguous pixels).  dt=np.float32 with C in f32 is the emulation of the stated
    operation order.  swap_t / no_hole_fallback / keep_eps: the planted defects."""
    N, _, H, W = S.shape
    left, right, tw = tables(keys, N)
    E = np.zeros((N, 2, H, W)) if E is None else E
    amb = np.zeros((N, 2, H, W), dtype=bool) if amb is None else amb
    xs, ys = np.meshgrid(np.arange(W, dtype=dt), np.arange(H, dtype=dt))
    S, R, C = S.astype(dt), R.astype(dt), C.astype(dt)
    eps_, thr_ = dt(eps), dt(np.float32(thr))
    eps = float(eps_)
    out = np.zeros((N, 3, H, W), dtype=dt); holes = np.zeros(N, dtype=np.int64)
    bound = np.zeros((N, 3, H, W)); left_out = np.zeros((N, H, W), dtype=bool)
    for i in range(N):
        if left[i] == right[i]:
            out[i] = R[left[i]]
            continue
        tk = [dt(tw[0, i]), dt(tw[1, i])]
        if swap_t:
            tk = tk[::-1]
        G, eG, w, skip = [], [], [], amb[i, 0] | amb[i, 1]
        for k, key in enumerate((left[i], right[i])):
            Sk, Rk, c = S[keys[key]], R[key], C[i, k]
            qx, qy = xs + c[0], ys + c[1]
            s, r = bil(Sk, qx, qy, dt), bil(Rk, qx, qy, dt)
            m = np.abs(s - S[i]).max(axis=0)
            skip |= (c[2] == 1) & (np.abs(m.astype(np.float64) - float(thr_)) < DELTA)      # behind valid = 0 the photo gate decides nothing
            w.append(tk[k] * c[2] * (m < thr_).astype(dt))
            n_, d_ = r + eps_, s + eps_
            G.append(n_ / d_)
            if dt is np.float64:
                eqx, eqy = E[i, k] + U * np.abs(qx), E[i, k] + U * np.abs(qy)
                err = []
                for T, v in ((Sk, d_), (Rk, n_)):
                    Lx, Ly = lipschitz(T)
                    x0, _, y0, _, _, _ = _cell(qx, qy, H, W)
                    err.append(Lx[:, y0, x0] * eqx + Ly[:, y0, x0] * eqy + 10 * U * tap_max(T, qx, qy) + U * np.abs(v))
                ed, en = err
                eG.append((en + np.abs(G[k]) * ed) / np.maximum(d_ - ed, 1e-300) + U * np.abs(G[k]))
        wsum = w[0] + w[1]
        seen = wsum > 0
        ws = np.where(seen, wsum, 1)
        g = (w[0] * G[0] + w[1] * G[1]) / ws
        Gp = [(R[key] + eps_) / (S[keys[key]] + eps_) for key in (left[i], right[i])]
        gh = tk[0] * Gp[0] + tk[1] * Gp[1]
        if no_hole_fallback:
            gh = np.ones_like(gh)
        g = np.where(seen, g, gh)
        a_ = S[i] + eps_
        out[i] = a_ * g if keep_eps else a_ * g - eps_
        holes[i] = int((~seen).sum())
        if dt is np.float64:
            eg = np.where(seen, (w[0] * eG[0] + w[1] * eG[1]) / ws + 5 * U * (w[0] * np.abs(G[0]) + w[1] * np.abs(G[1])) / ws,
                          6 * U * (tk[0] * np.abs(Gp[0]) + tk[1] * np.abs(Gp[1])))
            bound[i] = SAFETY * (np.abs(a_) * eg + 2 * U * np.abs(a_) * np.abs(g) + U * np.abs(out[i])) + 1e-12
            left_out[i] = skip
    return out, holes, bound, left_out


def chain_f32(fut, past, keys, alpha=ALPHA):
    """The chain in float32 in the stated operation order (numpy f32 arithmetic rounds every operation once, as the kernel without contraction)."""
    f = np.float32
    N, _, H, W = fut.shape
    xs, ys = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    C = np.zeros((N, 2, 3, H, W), dtype=f)
    al = f(alpha)
    for a, b in zip(keys, keys[1:]):
        for d in range(1, b - a):
            for direction, (j, own, back, prev) in enumerate(((a + d, past, fut, a + d - 1), (b - d, fut, past, b - d + 1))):
                A = own[j]
                qx, qy = xs + A[0], ys + A[1]
                g = bil(back[prev], qx, qy, f)
                ex, ey = A[0] + g[0], A[1] + g[1]
                lhs = ex * ex + ey * ey
                t = al * (np.sqrt(A[0] * A[0] + A[1] * A[1]) + np.sqrt(g[0] * g[0] + g[1] * g[1])) + al
                valid = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1) & (lhs < t * t)
                cx, cy = A[0], A[1]
                if d > 1:
                    P = C[prev, direction]
                    cx, cy = A[0] + bil(P[0], qx, qy, f), A[1] + bil(P[1], qx, qy, f)
                    v4, _, _ = taps(P[2], qx, qy)
                    valid &= (v4[0] == 1) & (v4[1] == 1) & (v4[2] == 1) & (v4[3] == 1)
                C[j, direction] = np.stack([np.where(valid, cx, f(0)), np.where(valid, cy, f(0)), valid.astype(f)])
    return C


# ------------------------------------------------------------------------------------------------------------------ inputs
def _texture(rng, h, w, waves=6, lo=0.05, hi=0.95):
    """A smooth random texture [3, h, w] in [lo, hi]: a few sinusoids per channel (largest neighbour difference around 0.1)."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    t = np.zeros((3, h, w))
    for c in range(3):
        for _ in range(waves):
            fx, fy, ph = rng.uniform(-0.35, 0.35), rng.uniform(-0.35, 0.35), rng.uniform(0, 2 * np.pi)
            t[c] += np.sin(fx * x + fy * y + ph)
    t = (t - t.min()) / (t.max() - t.min())
    return lo + (hi - lo) * t


def _smooth_field(rng, H, W, amp):
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = np.zeros((2, H, W))
    for c in range(2):
        for _ in range(3):
            f[c] += np.sin(rng.uniform(-0.08, 0.08) * x + rng.uniform(-0.08, 0.08) * y + rng.uniform(0, 2 * np.pi))
    return f * (amp / 3.0)


_CACHE = {}


def inputs(name):
    """-> dict(S [N,3,H,W], R [M,3,H,W], fut, past [N,2,H,W], keys), all float32.  integer: per-frame constant integer translations (some leave the
    frame); lattice: multiples of 1/4; smooth: a low-frequency field below 6 px, the backward flow its numeric inverse, plus a planted inconsistent
    patch in one backward flow and a planted photometric mismatch in one source frame."""
    N, K, H, W, family = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    keys = keyframe_ids(N, K)
    pad = 100
    canvas = _texture(rng, H + 2 * pad, W + 2 * pad)
    gain = 0.5 + _texture(rng, H + 2 * pad, W + 2 * pad, waves=3, lo=0.0, hi=1.0)[:1]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fut = np.zeros((N, 2, H, W)); past = np.zeros((N, 2, H, W))
    S = np.zeros((N, 3, H, W)); Gn = np.zeros((N, 1, H, W))
    if family in ("integer", "lattice"):
        # frame i shows the canvas at offset o_i: content at p in frame i sits at p + (o_i - o_{i+1}) in frame i+1
        step = 1.0 if family == "integer" else 0.25
        lim = min(3.0, (H - 1) / 2.0) if family == "integer" else 1.5
        v = np.round(rng.uniform(-lim, lim, size=(N, 2)) / step) * step
        v[:, 0] = np.round(rng.uniform(-5, 5, size=N) / step) * step            # x: up to 5 px per frame, so content leaves the frame
        o = np.concatenate([[[0.0, 0.0]], -np.cumsum(v[:-1], axis=0)]) + pad
        for i in range(N):
            S[i] = bil(canvas, xx + o[i, 0], yy + o[i, 1])
            Gn[i] = bil(gain, xx + o[i, 0], yy + o[i, 1])
            if i + 1 < N:
                fut[i] = v[i][:, None, None]
                past[i + 1] = -v[i][:, None, None]
    else:
        amp = min(4.0, H / 3.0)
        S[0] = canvas[:, pad:pad + H, pad:pad + W]
        Gn[0] = gain[:, pad:pad + H, pad:pad + W]
        for i in range(N - 1):
            fut[i] = _smooth_field(rng, H, W, amp)
            b = -fut[i]
            for _ in range(4):                                                  # past[i+1](p) = -fut[i](p + past[i+1](p))
                b = -bil(fut[i], xx + b[0], yy + b[1])
            past[i + 1] = b
            S[i + 1] = bil(S[i], xx + b[0], yy + b[1])
            Gn[i + 1] = bil(Gn[i], xx + b[0], yy + b[1])
        j = keys[0] + 1 if N > 2 else 1
        past[j, 0, H // 4:H // 2, W // 4:W // 2] += 3.0                          # inconsistent with fut[j-1]: fb fails there
        past[j, 1, H // 4:H // 2, W // 4:W // 2] -= 2.0
        S[j, :, H // 2:3 * H // 4, W // 2:3 * W // 4] += 0.3                     # photometric mismatch against both keys: holes
    S = S.astype(np.float32)
    R = (S[keys] * Gn[keys].astype(np.float32)).astype(np.float32)
    return dict(S=S, R=R, fut=fut.astype(np.float32), past=past.astype(np.float32), keys=keys)


def case(name):
    """inputs(name) plus the float64 reference: C, E, amb of the chain; out, holes, bound, left_out of the propagation.  Computed once."""
    if name not in _CACHE:
        c = inputs(name)
        c["C"], c["E"], c["amb"] = chain_ref(c["fut"], c["past"], c["keys"])
        c["out"], c["holes"], c["bound"], c["left_out"] = propagate_ref(c["S"], c["R"], c["keys"], c["C"], c["E"], c["amb"])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------------------------ exact planted motion
def planted_bound(v, eps=EPS):
    """Test 1 (integer motion, relit key = f32(source * gain), the gain moving with the texture): both keys see s = S_i(p) exactly and r = f32(s g), so
    G_a = G_b and out = (s + eps) G - eps is r up to the roundings of r itself (1), r + eps, s + eps, the division (3), the two products, the sum and
    the division of the blend (4), the last product and subtraction (2): 10 roundings of quantities no larger than |v| + eps each, amplified by at
    most (s + eps) / (s + eps) = 1  ->  12 U (|v| + eps) with a margin of two roundings."""
    return 12 * U * (np.abs(v) + eps)
