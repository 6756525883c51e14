"""References, inputs and case tables of the leaf parity tests of the correlation lookup and the RAFT update kernels (tests/test_gpu_flow_leaves.py;
pinned on the CPU by tests/test_flow_refs_cpu.py).  torch on the CPU only; tolerances and helpers are those of tests/leaf_refs.py.

Every `*_ref(..., dt)` evaluates one operation in the dtype `dt` on the kernel's own rounded inputs: dt = float64 is the reference, dt = float32 the same
operation at the precision the kernels accumulate in (the elementwise atol of an f16 output is 4 x their largest difference, leaf_refs.floor_atol).
Layouts are the kernels': NHWC feature maps and rows, coords [B,2,H,W] (x, y), tap-major weights.
"""
import math

import torch
import torch.nn.functional as F

from leaf_refs import (ATOL_CAP, F32, F64, H, REL_F16, avgpool2_nhwc_ref, elem_excess, f32_tol, floor_atol, rel_l2, rng,  # noqa: F401 (re-exported)
                       sentinel16)


# ------------------------------------------------------------------------------------------------------------------ correlation lookup
def corr_ref(f1, levels, coords, r, dt):
    """The window lookup from its definition (csrc/flow.hip, k_corr_lookup): f1 [B,H,W,D], levels[l] [B,Hl,Wl,D] (the pyramid the kernel reads),
    coords [B,2,H,W] (x, y) -> [B, H*W, L*n*n], n = 2r + 1, channel (l*n + a)*n + b2 = the all-pairs correlation <f1[p], levels[l][.]> sampled
    bilinearly with zero padding at (x / 2^l + a - r, y / 2^l + b2 - r), times 1/sqrt(D)."""
    B, Hh, Ww, D = f1.shape
    P, n = Hh * Ww, 2 * r + 1
    q = f1.to(dt).reshape(B, P, D)
    off = torch.arange(-r, r + 1)
    out = []
    for l, g in enumerate(levels):
        Hl, Wl = g.shape[1:3]
        vol = torch.bmm(q, g.to(dt).reshape(B, Hl * Wl, D).transpose(1, 2))                  # [B, P, Hl*Wl]
        cx, cy = coords[:, 0].reshape(B, P).to(dt) / 2 ** l, coords[:, 1].reshape(B, P).to(dt) / 2 ** l
        # the offsets are integers: the sample (cx + a - r, cy + b2 - r) has the fraction of the centre and the floor floor(cx) + a - r
        fx, fy = (cx - torch.floor(cx))[:, :, None, None], (cy - torch.floor(cy))[:, :, None, None]
        x0 = (torch.floor(cx).long()[:, :, None, None] + off[None, None, :, None]).expand(B, P, n, n)       # index a: x offset
        y0 = (torch.floor(cy).long()[:, :, None, None] + off[None, None, None, :]).expand(B, P, n, n)       # index b2: y offset
        v = torch.zeros(B, P, n, n, dtype=dt)
        for dy, dx, wgt in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
            ix, iy = x0 + dx, y0 + dy
            ok = (ix >= 0) & (ix < Wl) & (iy >= 0) & (iy < Hl)
            idx = (iy.clamp(0, Hl - 1) * Wl + ix.clamp(0, Wl - 1)).reshape(B, P, n * n)
            v = v + wgt * torch.gather(vol, 2, idx).reshape(B, P, n, n) * ok
        out.append(v.reshape(B, P, n * n))
    return torch.cat(out, 2) * (1.0 / math.sqrt(D))


def lattice_map(B, Hh, Ww, D, seed):
    """[B,H,W,D] f32 on the lattice k/8, |k| <= 32: every 2x2-mean level down to level 3 has a numerator <= 2^11 over 512 -- exact in f32 and f16."""
    return torch.randint(-32, 33, (B, Hh, Ww, D), generator=rng(seed)).to(F32) / 8


def pyramid(f2, num_levels):
    """The f32 2x2-mean pyramid (floor halving, as tcl_avgpool2_nhwc_f32 pools): [f2, ...]."""
    lv = [f2]
    for _ in range(num_levels - 1):
        lv.append(avgpool2_nhwc_ref(lv[-1], F32))
    return lv


def grid(B, Hh, Ww):
    ys, xs = torch.meshgrid(torch.arange(Hh).float(), torch.arange(Ww).float(), indexing="ij")
    return torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)


CORR_D, CORR_R, CORR_B = (64, 192, 256, 512), (1, 4, 5), (1, 2)
CORR_SHAPES = ((5, 7, 3), (9, 13, 4), (16, 24, 4), (4, 4, 1))          # H, W, levels: P % 4 != 0, 1x1 coarsest levels, odd sizes that drop a row / column
CORR_COORDS = ("noise", "integer", "half", "outside", "border")
ROWS_D, ROWS_R = (192, 256), (1, 4)                                     # tcl_corr_lookup_rows_f16: ld = 384 and ld = L*n*n, B = 2


def corr_coords(kind, B, Hh, Ww, r, levels, seed):
    """coords [B,2,H,W] f32 of one coordinate set."""
    g, c = rng(seed), grid(B, Hh, Ww)
    if kind == "noise":                                                  # grid + N(0, 2)
        return c + 2 * torch.randn(B, 2, Hh, Ww, generator=g)
    if kind == "integer":                                                # fx = fy = 0
        return c + torch.randint(-3, 4, (B, 2, Hh, Ww), generator=g).float()
    if kind == "half":                                                   # exact half-integers; the first column / row negative (floorf != truncation)
        c = c + torch.randint(-3, 4, (B, 2, Hh, Ww), generator=g).float() + 0.5
        c[:, 0, :, 0] = -0.5 - torch.arange(Hh).float() % 3
        c[:, 1, 0, :] = -1.5 - torch.arange(Ww).float() % 2
        return c
    if kind == "outside":                                                # every window more than r + 1 outside at every level; left / right / above / below
        m = float((2 * r + 3) * 2 ** (levels - 1))
        k = torch.arange(Hh * Ww).view(Hh, Ww)
        far = torch.rand(B, Hh, Ww, generator=g) * 3
        c[:, 0] = torch.where(k % 4 == 0, -m - far, torch.where(k % 4 == 1, Ww + m + far, c[:, 0]))
        c[:, 1] = torch.where(k % 4 == 2, -m - far, torch.where(k % 4 == 3, Hh + m + far, c[:, 1]))
        return c
    assert kind == "border"                                              # windows hanging over each border, the rest near the grid
    c = c + torch.randn(B, 2, Hh, Ww, generator=g)
    c[:, 0, :, 0] = -r + 0.3
    c[:, 0, :, -1] = Ww - 1 + r - 0.25
    c[:, 1, 0, :] = -0.75
    c[:, 1, -1, :] = Hh - 0.5 + 0.125 * torch.arange(Ww).float()
    return c


def corr_input(D, Hh, Ww, levels, r, kind, B=2):
    """-> (f1 [B,H,W,D], pyramid levels, coords): seeded lattice maps, one pair per (D, H, W), and one coordinate set."""
    f1, f2 = lattice_map(B, Hh, Ww, D, D + Hh), lattice_map(B, Hh, Ww, D, D + Hh + 1)
    return f1, pyramid(f2, levels), corr_coords(kind, B, Hh, Ww, r, levels, Hh * Ww + r + CORR_COORDS.index(kind))


# ---- the tile-sharing kernel: its band / flag decisions restated on the host
TILED_D, TILED_SHAPES, TILED_COORDS = (64, 256), ((9, 13), (16, 24), (17, 25)), ("smooth", "zoom", "torn")
TILED_BIG = (64, 72)       # fmap2 of the zoom and torn sets.  The kernel clips a tile's box to the level, and a map of at most 17 x 25 = 425 points
#                            fits one band of CT_RMAX = 512: more than one band, or a raised flag, needs a larger fmap2 (the ABI takes its size per level)
CT_RMAX, CT_MAXB = 512, 8


def tiled_input(D, Hh, Ww, kind):
    """-> (f1 [1,H,W,D], pyramid levels of fmap2, coords [1,2,H,W])."""
    g = rng(D + Hh + TILED_COORDS.index(kind))
    H2, W2 = (Hh, Ww) if kind == "smooth" else TILED_BIG
    f1, f2 = lattice_map(1, Hh, Ww, D, D + Hh + 2), lattice_map(1, H2, W2, D, D + Hh + 3)
    c = grid(1, Hh, Ww)
    xs, ys = c[:, 0].clone(), c[:, 1].clone()
    if kind == "zoom":                                                   # a 2.6x zoom: an 8 x 8 tile's windows span 29 x 29 = 841 points -> two bands
        c = c * 2.6 + torch.tensor([3.2, 2.7]).view(1, 2, 1, 1)
    else:
        c = c + torch.stack([1.3 + 0.8 * torch.sin(xs / 5 + ys / 7), -0.7 + 0.6 * torch.cos(ys / 4)], 1)
    if kind == "torn":
        c = c + torch.tensor([20.3, 15.6]).view(1, 2, 1, 1)
        c[:, 0, :8, :8] = torch.rand(1, 8, 8, generator=g) * W2         # tile 0 torn over the whole map: 64 x 72 points > CT_MAXB bands of 7 rows
        c[:, 1, :8, :8] = torch.rand(1, 8, 8, generator=g) * H2
        c[:, 0, :, -1] = W2 - 0.5 - 0.25 * torch.arange(Hh).float()      # windows over the right and the upper border
        c[:, 1, 0, 8:] = -2.5
    return f1, pyramid(f2, 4), c.contiguous()


def tile_bands(coords, level_hw, r=4):
    """Staging bands per (level, 8x8 tile) as k_corr_lookup_tile decides them: 0 = empty box, > CT_MAXB = flag raised.  -> int tensor [L, tiles]."""
    _, _, Hh, Ww = coords.shape
    ty, tx = (Hh + 7) // 8, (Ww + 7) // 8
    out = torch.zeros(len(level_hw), ty * tx, dtype=torch.int64)
    for l, (Hl, Wl) in enumerate(level_hw):
        x0 = torch.floor(coords[0, 0] / 2 ** l).long() - r
        y0 = torch.floor(coords[0, 1] / 2 ** l).long() - r
        for t in range(ty * tx):
            sy, sx = slice((t // tx) * 8, (t // tx) * 8 + 8), slice((t % tx) * 8, (t % tx) * 8 + 8)
            mnx, mxx = max(int(x0[sy, sx].min()), 0), min(int(x0[sy, sx].max()) + 2 * r + 1, Wl - 1)
            mny, mxy = max(int(y0[sy, sx].min()), 0), min(int(y0[sy, sx].max()) + 2 * r + 1, Hl - 1)
            bw, bh = mxx - mnx + 1, mxy - mny + 1
            if bw > 0 and bh > 0:
                rows = CT_RMAX // bw
                out[l, t] = -(-bh // rows) if rows > 0 else CT_MAXB + 1
    return out


# ------------------------------------------------------------------------------------------------------------------ SepConvGRU half-steps
def sepconv_ref(src0, src1, W, Hh, Wd, vertical, dt):
    """The 1x5 (pad (0,2)) / 5x1 (pad (2,0)) convolution over x = [src0 | src1] rows [M,128] each (src1 may be None): W [N, 5*(128 + C1)] with column
    tap*(128 + C1) + source*128 + c -> [M, N]."""
    x = src0.to(dt) if src1 is None else torch.cat([src0.to(dt), src1.to(dt)], 1)
    M, C = x.shape
    x = x.view(M // (Hh * Wd), Hh, Wd, C)
    ax, ext = (1, Hh) if vertical else (2, Wd)
    cols = []
    for tap in range(5):
        d, sh = tap - 2, torch.zeros_like(x)
        lo, hi = max(0, -d), min(ext, ext - d)                           # output positions whose tap lies inside
        if hi > lo:
            sh.narrow(ax, lo, hi - lo).copy_(x.narrow(ax, lo + d, hi - lo))
        cols.append(sh)
    return torch.cat(cols, 3).reshape(M, 5 * C) @ W.to(dt).t()


def fold_ref(src0, src1, W, bias, Hh, Wd, vertical, dt):
    """mode 0: the convolution + the channel bias, f32 out."""
    return sepconv_ref(src0, src1, W, Hh, Wd, vertical, dt) + bias.to(dt)


def gate_ref(h, mot, W, pb, Hh, Wd, vertical, dt):
    """mode 1: v = conv([h | mot]) + pb [M,256] -> z = sigmoid(v[:, :128]) (f32 out), rh = sigmoid(v[:, 128:]) * h (f16 out)."""
    g = torch.sigmoid(sepconv_ref(h, mot, W, Hh, Wd, vertical, dt) + pb.to(dt))
    return g[:, :128], g[:, 128:] * h.to(dt)


def gate_rh_ref(h, mot, W, pb, Hh, Wd, vertical, dt):
    return gate_ref(h, mot, W, pb, Hh, Wd, vertical, dt)[1]


def cand_ref(rh, mot, W, pb, z, h, Hh, Wd, vertical, dt):
    """mode 2: q = tanh(conv([rh | mot]) + pb [M,128]); -> (1 - z) h + z q with the f32 z given (f16 out)."""
    q = torch.tanh(sepconv_ref(rh, mot, W, Hh, Wd, vertical, dt) + pb.to(dt))
    return (1 - z.to(dt)) * h.to(dt) + z.to(dt) * q


SEP_SHAPES = ((1, 16, 16), (1, 5, 13), (2, 3, 7), (3, 9, 7), (1, 1, 4))          # B, H, W: M = 256 / 65 / 42 / 189 / 4
SEP_CONFIGS = (("fold", 0, 128, 0), ("fold", 0, 256, 0), ("fold", 0, 128, 128), ("gate", 1, 256, 128), ("cand", 2, 128, 128))    # name, mode, N, C1


def sep_input(B, Hh, Wd, N, C1, seed):
    """Activations as the engine's (tanh / relu of N(0,1)), weights ~ N(0, 1/K): dict of s0, s1 (None at C1 = 0), w, bias [N], pb [M,N], z, h."""
    g, M, K = rng(seed), B * Hh * Wd, 5 * (128 + C1)
    return dict(s0=torch.tanh(torch.randn(M, 128, generator=g)).to(H), s1=torch.relu(torch.randn(M, 128, generator=g)).to(H) if C1 else None,
                w=(torch.randn(N, K, generator=g) / K ** 0.5).to(H), bias=0.5 * torch.randn(N, generator=g), pb=0.5 * torch.randn(M, N, generator=g),
                z=torch.sigmoid(torch.randn(M, 128, generator=g)), h=torch.tanh(torch.randn(M, 128, generator=g)).to(H))


def sep_case(name, N, C1, B, Hh, Wd, vertical):
    """-> (inputs, ref_fn, args) of one case; the f16 output of `gate` is rh (gate_rh_ref)."""
    i = sep_input(B, Hh, Wd, N, C1, 1000 * N + 10 * C1 + B * Hh * Wd + vertical)
    if name == "fold":
        return i, fold_ref, (i["s0"], i["s1"], i["w"], i["bias"], Hh, Wd, vertical)
    if name == "gate":
        return i, gate_rh_ref, (i["h"], i["s1"], i["w"], i["pb"], Hh, Wd, vertical)
    return i, cand_ref, (i["s0"], i["s1"], i["w"], i["pb"], i["z"], i["h"], Hh, Wd, vertical)


# ------------------------------------------------------------------------------------------------------------------ convf1
def convf1_ref(coords1, w_t, bias, dt):
    """relu(Conv2d(2, 128, 7, padding=3)(coords1 - pixel grid)): the subtraction in f32 as the kernel does it, the rest in dt.  coords1 [B,2,H,W],
    w_t [98,128] with row c*49 + ky*7 + kx -> rows [B*H*W, 128]."""
    B, _, Hh, Ww = coords1.shape
    flow = (coords1.float() - grid(B, Hh, Ww)).to(dt)
    cols = F.unfold(flow, 7, padding=3).transpose(1, 2).reshape(B * Hh * Ww, 98)
    return torch.relu(cols @ w_t.to(dt) + bias.to(dt))


CONVF1_CASES = ((1, 3, 5, 128), (2, 7, 11, 136), (1, 8, 8, 128))                  # B, H, W, ldo
CONVF1_COORDS = ("noise", "far")


def convf1_input(B, Hh, Ww, kind):
    g = rng(B + Hh + Ww + CONVF1_COORDS.index(kind))
    w = torch.randn(128, 2, 7, 7, generator=g) / 98 ** 0.5
    d = 3 * torch.randn(B, 2, Hh, Ww, generator=g) if kind == "noise" else 800 * torch.rand(B, 2, Hh, Ww, generator=g) - 400      # flows of a few hundred pixels
    return (grid(B, Hh, Ww) + d).contiguous(), w.reshape(128, 98).t().contiguous(), 0.5 * torch.randn(128, generator=g)


# ------------------------------------------------------------------------------------------------------------------ the cases of the f16 outputs
def f16_floor_cases():
    """Every (kernel, case id, ref_fn, args) whose output is f16: what test_flow_refs_cpu.py pins and the GPU tests take their atol from."""
    for D in ROWS_D:
        for Hh, Ww, lv in CORR_SHAPES:
            for r in ROWS_R:
                for kind in CORR_COORDS:
                    f1, levels, co = corr_input(D, Hh, Ww, lv, r, kind)
                    yield "corr_rows", (D, Hh, Ww, lv, r, kind), corr_ref, (f1, levels, co, r)
    for D in TILED_D:
        for Hh, Ww in TILED_SHAPES:
            for kind in TILED_COORDS:
                f1, levels, co = tiled_input(D, Hh, Ww, kind)
                yield "corr_tiled", (D, Hh, Ww, kind), corr_ref, (f1, levels, co, 4)
    for name, mode, N, C1 in SEP_CONFIGS:
        if mode:
            for B, Hh, Wd in SEP_SHAPES:
                for vertical in (0, 1):
                    _, fn, args = sep_case(name, N, C1, B, Hh, Wd, vertical)
                    yield "sepconv_" + name, (B, Hh, Wd, vertical), fn, args
    for B, Hh, Ww, _ in CONVF1_CASES:
        for kind in CONVF1_COORDS:
            yield "convf1", (B, Hh, Ww, kind), convf1_ref, convf1_input(B, Hh, Ww, kind)


_ATOL = {}


def atol_of(kernel, case):
    """floor_atol of one case of f16_floor_cases(), cached: -> (atol, rms)."""
    if not _ATOL:
        for name, cid, fn, args in f16_floor_cases():
            _ATOL[(name, cid)] = (fn, args)
    v = _ATOL[(kernel, tuple(case))]
    if callable(v[0]):
        v = _ATOL[(kernel, tuple(case))] = floor_atol(v[0], *v[1])
    return v
