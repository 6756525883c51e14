"""NumPy restatements of generation.normal (IC-Light's "Compute Normal", the background demo's process_normal): the matte with its sigma offset and
the normal from four directional relights -- once in float64 (the yardstick) and once in float32 numpy, operation by operation in the demo's order (what rounding
alone costs: the figure D the GPU test's tolerances are multiples of).  Restated from the header's comment and the demo, never from the kernel's
outputs.  The test inputs of tests/test_gpu_normal.py live here too, so that the CPU test can check them without a GPU."""
import functools

import numpy as np

F32 = np.float32
SIDES = ("left", "right", "bottom", "top")       # the demo's order
EPS = 1e-5
SHAPES = ((5, 7), (64, 64))                      # the scalar path (H*W % 4 != 0, more than one group per frame) and the 16 B path (more than one block)
N_FRAMES = 2


def matte_q(f, a, sigma=0.0):
    """The integer the matte stores, per element in f32 with every operation rounded on its own: u = 255 f; v = 127 + ((u - 127) + sigma) a;
    q = trunc(clamp(v, 0, 255)), NaN -> 0.  f, a: arrays broadcast against each other."""
    f, a = np.asarray(f, dtype=F32), np.asarray(a, dtype=F32)
    u = (F32(255.0) * f).astype(F32)
    d = ((u - F32(127.0)).astype(F32) + F32(sigma)).astype(F32)
    m = (d * a).astype(F32)
    v = (F32(127.0) + m).astype(F32)
    v = np.where(np.isnan(v), F32(0.0), v)
    return np.trunc(np.clip(v, F32(0.0), F32(255.0))).astype(np.int64)


def _clamp01(x):
    """The kernel's input clamp on the f32 values: [0, 1], NaN -> 0 (exact in any precision)."""
    x = np.asarray(x, dtype=F32)
    return np.clip(np.where(np.isnan(x), F32(0.0), x), F32(0.0), F32(1.0))


def matte_k(alpha, shape):
    """The integer of the demo's u8 round trip of the matte, k = trunc(clamp(fl32(alpha * 255), 0, 255)), NaN -> 0; None: 255 everywhere.  The
    product is the f32 one in both restatements: k is a discrete choice, not a rounding error."""
    if alpha is None:
        return np.full(shape, 255, dtype=np.int64)
    v = (np.asarray(alpha, dtype=F32) * F32(255.0)).astype(F32)
    v = np.where(np.isnan(v), F32(0.0), v)
    return np.trunc(np.clip(v, F32(0.0), F32(255.0))).astype(np.int64)


def normal_f64(left, right, bottom, top, alpha=None):
    """The formula in float64 on the f32 inputs [n,3,H,W] (alpha [n,1,H,W] or None).  -> dict(normal [n,3,H,W] f64, ambient [n,3,H,W] f64,
    y [n,H,W,3] f64: out * 127.5 + 127.5 clamped to [0, 255], the value whose truncation is normal_u8)."""
    L, R, B, T = (_clamp01(x).astype(np.float64) for x in (left, right, bottom, top))
    e = np.float64(F32(EPS))
    A = (L + R + B + T) * 0.25
    q = lambda X: (X + e) / (A + e) - 1.0
    u = ((q(R) - q(L)) * 0.5).sum(axis=1) / 3.0
    v = ((q(T) - q(B)) * 0.5).sum(axis=1) / 3.0
    s = np.clip(1.0 - u * u - v * v, 0.0, 1e5)
    h = s ** 5
    N = np.stack([u, v, h], axis=1) / np.sqrt(u * u + v * v + h * h)[:, None]
    m = matte_k(alpha, (L.shape[0], 1) + L.shape[2:]).astype(np.float64) / 255.0
    up = np.zeros_like(N)
    up[:, 2] = 1.0
    out = N * m + up * (1.0 - m)
    y = np.clip(out * 127.5 + 127.5, 0.0, 255.0).transpose(0, 2, 3, 1)
    return dict(normal=out, ambient=A, y=np.ascontiguousarray(y))


def normal_f32(left, right, bottom, top, alpha=None):
    """The formula on float32 numpy arrays [n,3,H,W], every operation rounded to f32 on its own, in the order IC-Light's demo applies them: the four
    relights summed one after the other and divided by 4.0; the ratio to that mean less one; half the right-left and top-bottom differences;
    np.mean over the channel axis; squares as `** 2.0`; the fifth power as `** 5.0`; the length as the channel sum of squares `** 0.5`; the
    blend with the matte k/255.  -> dict(normal [n,3,H,W] f32, ambient [n,3,H,W] f32)."""
    rel = [_clamp01(x) for x in (left, right, bottom, top)]
    n, _, H, W = rel[0].shape
    ambient = (rel[0] + rel[1] + rel[2] + rel[3]) / 4.0
    ratio = [(x + EPS) / (ambient + EPS) - 1.0 for x in rel]                      # left, right, bottom, top
    u = np.mean((ratio[1] - ratio[0]) * 0.5, axis=1)
    v = np.mean((ratio[3] - ratio[2]) * 0.5, axis=1)
    h = np.clip(1.0 - u ** 2.0 - v ** 2.0, 0, 1e5) ** 5.0
    vec = np.stack([u, v, h], axis=1)
    vec = vec / np.sum(vec ** 2.0, axis=1, keepdims=True) ** 0.5
    m = matte_k(alpha, (n, 1, H, W)).astype(F32) / F32(255.0)
    viewer = np.zeros_like(vec)
    viewer[:, 2] = 1.0
    out = vec * m + viewer * (1 - m)
    assert out.dtype == F32 and ambient.dtype == F32
    return dict(normal=np.ascontiguousarray(out), ambient=np.ascontiguousarray(ambient))


def kernel_inputs(H, W, n=N_FRAMES):
    """The general case of the kernel test: a random image in [0.2, 0.8] seen under four lights that move every value by up to 0.15 (what four
    relights of one foreground look like: |u|, |v| stay below 1 almost everywhere, so h is a generic number rather than the clamp's 0), a dozen
    values outside [0, 1] on either side in every relight, one NaN, a pixel whose four relights are all below 0 (A = 0), and an alpha uniform in
    [0.05, 1] with a few exact 0, 1 and one NaN.  The seed depends on the shape only; test_normal_refs_cpu.py checks that these inputs keep clear
    of the u8 truncation boundaries (an alpha below 1/255 or h = 0 puts the third channel on an integer or close to one: 255, or 255 - k/2)."""
    rng = np.random.default_rng(7000 + 100 * H + W)
    base = rng.uniform(0.2, 0.8, size=(n, 3, H, W))
    rel = [(base + rng.uniform(-0.15, 0.15, size=base.shape)).astype(F32) for _ in SIDES]
    for x in rel:
        flat = x.reshape(-1)
        idx = rng.choice(flat.size, size=12, replace=False)
        flat[idx[:6]] = rng.uniform(-0.5, -0.01, size=6).astype(F32)
        flat[idx[6:]] = rng.uniform(1.01, 1.5, size=6).astype(F32)
    rel[1][0, 1, 2, 3] = np.nan
    for x in rel:
        x[1, :, 1, 1] = F32(-0.1)
    alpha = (0.05 + 0.95 * rng.random((n, 1, H, W))).astype(F32)
    alpha[0, 0, 0, :3] = [0.0, 1.0, np.nan]
    alpha[1, 0, -1, -2:] = [1.0, 0.0]
    return rel, alpha


@functools.lru_cache(maxsize=None)
def parity():
    """Computed once: per shape the inputs, the float64 and the float32 numpy results, and D = the largest |normal_f32 - normal_f64| over all
    of them (what float32 rounding alone costs on these inputs)."""
    cases, D = {}, 0.0
    for H, W in SHAPES:
        rel, alpha = kernel_inputs(H, W)
        r64, r32 = normal_f64(*rel, alpha), normal_f32(*rel, alpha)
        D = max(D, float(np.abs(r32["normal"].astype(np.float64) - r64["normal"]).max()))
        cases[(H, W)] = dict(rel=rel, alpha=alpha, f64=r64, f32=r32)
    return cases, D


def near_integer(y, margin):
    """[n,H,W] bool: a pixel with a channel whose pre-truncation value lies within `margin` of an integer."""
    return (np.abs(y - np.rint(y)) <= margin).any(axis=-1)
