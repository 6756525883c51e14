"""Plain CPU references and generators for the exact leaf parity tests of tcl_gemm_f16 / tcl_conv3x3_f16 (tests/test_gpu_gemm_leaves.py); pinned to
torch float64 by tests/test_gemm_refs_cpu.py.  numpy / torch CPU only.

The idea: f16 operands on a small lattice (integers, or multiples of 1/8) make every product and every f32 partial sum of a GEMM exact, in any summation
order and with any K split, so a kernel owes the reference's numbers bit for bit, element by element.  assert_exact_ok states the condition; the
generators meet it for every case of CASES (asserted on the CPU), so the GPU test never leaves an element out.

Epilogue of the kernels (csrc/gemm.hip), which the references follow: t = f16(act(acc + bias)); C = f16(post(t + resid)), act 1 SiLU, 3 ReLU, 4 erf-GELU,
5 = erf-GELU applied AFTER the residual (post), 2 = GEGLU: C = f16(f16(value) * gelu(f16(gate))) on the [value | gate] halves of the columns."""
import math

import numpy as np
import torch

H = torch.float16
FORCED = (1, 2, 3, 4, 11, 5, 6, 7, 8, 12, 13, 14, 15, 9, 10)      # the tcl_gemm_tune ids of csrc/gemm.hip: g_tiles
DMA = (1, 2, 3, 4, 11)                                              # the tiles with a K split
INT_A, INT_W, INT_B = tuple(range(-2, 3)), (-1, 0, 1), tuple(range(-4, 5))
EIGHTHS = tuple(v / 8 for v in range(-4, 5))                       # A of the non-linear cases: z stays where the activations bend


def lattice(shape, vals, p_zero, seed):
    """f16 tensor with entries drawn uniformly from vals (exactly representable values); a share p_zero of the entries is set to zero on top."""
    g = np.random.default_rng(seed)
    v = np.asarray(vals, dtype=np.float64)
    x = v[g.integers(0, len(v), size=shape)]
    x[g.random(size=shape) < p_zero] = 0.0
    t = torch.from_numpy(np.ascontiguousarray(x)).to(H)
    assert torch.equal(t.double(), torch.from_numpy(x))
    return t


def ulp_f16(x):
    """Spacing of f16 at |x| (float64 tensor in, float64 out): 2^(floor(log2|x|) - 10), the subnormal spacing 2^-24 as the floor."""
    a = torch.as_tensor(x, dtype=torch.float64).abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10).clamp_min(2.0 ** -24)


def _acc(A, W, den):
    """A . W^T without rounding: int64 on the integer lattice, float64 (exact: every value is a multiple of 1/den^2 far below 2^53) otherwise."""
    if den == 1:
        return (A.to(torch.int64) @ W.to(torch.int64).t()).double()
    return A.double() @ W.double().t()


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _act64(z, act):
    return {0: z, 1: z * torch.sigmoid(z), 3: z.clamp_min(0.0), 4: gelu64(z), 5: z}[act]


def _epilogue(acc, bias, resid, act):
    """-> (result, z, staged), float64.  z: the argument of the activation (acc + bias; with act 5 the staged f16 value + resid); staged: what the kernels
    round to f16 BEFORE the residual is added (None without a residual) -- exactness needs it representable."""
    z = acc + (bias.double() if bias is not None else 0.0)
    if act == 2:
        D = z.shape[-1] // 2
        return z[..., :D] * gelu64(z[..., D:]), z, z
    if resid is None:
        return (gelu64(z) if act == 5 else _act64(z, act)), z, None
    if act == 5:
        return gelu64(z + resid.double()), z + resid.double(), z
    return _act64(z, act) + resid.double(), z, _act64(z, act)


def gemm_exact(A, W, bias, resid, act, den=1):
    """C = epilogue(A[M,K] . W[N,K]^T): -> (result, z, staged) in float64 (see _epilogue).  act 2: W / bias in the [value (N/2) | gate (N/2)] row order."""
    return _epilogue(_acc(A, W, den), bias, resid, act)


def nearest_src(n_in, n_up):
    """Source index of every up-sampled position: min(floor(y * (float)n_in / (float)n_up), n_in - 1) in f32, PyTorch's 'nearest' rule."""
    s = np.float32(n_in) / np.float32(n_up)
    return np.minimum(np.floor(np.arange(n_up, dtype=np.float32) * s).astype(np.int64), n_in - 1)


def conv_out_hw(Hup, Wup, stride, pad):
    return ((Hup + 2 - 3) // stride + 1, (Wup + 2 - 3) // stride + 1) if pad else ((Hup + 1 - 3) // stride + 1, (Wup + 1 - 3) // stride + 1)


def conv3x3_exact(X, W, bias, resid, stride, pad, Hup, Wup, act, den=1):
    """3x3 convolution from its definition.  X [B, Hin, Win, Cin] NHWC; W [Cout, 9 * Cin] tap-major (tap = 3 * ky + kx); the input is first up-sampled
    to Hup x Wup by nearest_src (0: keep), then zero-padded: one pixel all round for pad = 1, one row below and one column right ((0, 1, 0, 1)) for
    pad = 0; output pixel (oy, ox) sums padded[oy * stride + ky, ox * stride + kx, ci] * W[co, tap, ci].  resid [B, Hout, Wout, Cout].
    -> (result, z, staged) in float64, NHWC."""
    B, Hin, Win, Cin = X.shape
    Cout = W.shape[0]
    Hup, Wup = Hup or Hin, Wup or Win
    up = X[:, torch.from_numpy(nearest_src(Hin, Hup))][:, :, torch.from_numpy(nearest_src(Win, Wup))]
    padded = torch.zeros(B, Hup + (2 if pad else 1), Wup + (2 if pad else 1), Cin, dtype=X.dtype)
    o = 1 if pad else 0
    padded[:, o:o + Hup, o:o + Wup] = up
    Ho, Wo = conv_out_hw(Hup, Wup, stride, pad)
    acc = torch.zeros(B * Ho * Wo, Cout, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            patch = padded[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            tap = 3 * ky + kx
            acc += _acc(patch.reshape(-1, Cin), W[:, tap * Cin:(tap + 1) * Cin], den)
    return _epilogue(acc.view(B, Ho, Wo, Cout), bias, resid, act)


def f16_exact(t):
    return bool((t.to(H).double() == t).all())


def assert_exact_ok(z, out, den=1, linear=True, staged=None):
    """The condition under which bit equality with the reference is owed: every pre-activation value is on the lattice (a multiple of 1/den) with
    |z| < 2^24 / den -- with operands bounded as the generators bound them this makes every f32 partial sum exact, in any order; what the kernel rounds
    to f16 before the residual (staged) is representable; and every linear-epilogue result (act 0 / 3) is an integer of magnitude <= 2048."""
    assert bool(((z * den) == torch.round(z * den)).all()), "pre-activation off the lattice"
    assert float(z.abs().max()) < 2.0 ** 24 / den
    if staged is not None:
        assert f16_exact(staged), "the value staged in f16 before the residual is not representable"
    if linear:
        assert bool((out == torch.round(out)).all()) and float(out.abs().max()) <= 2048.0, "a linear result is not an integer of magnitude <= 2048"
        assert f16_exact(out)


def ceil64(n):
    return (n + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------------------------------------------------------- cases
# must_run: the forced tile ids (of `cfgs`, default FORCED) that the dispatcher accepts for the case -- recorded from tcl_gemm_plan / tcl_conv3x3_plan
# under tcl_gemm_tune and asserted by test_gemm_refs_cpu.py, so that the GPU test cannot pass by skipping a tile.
# Dense: resid 0 none, 1 a separate tensor, 2 in place (resid is C); ld* None = tight; vae: A and W are the first two column thirds of one [M, 3K]
# buffer (M == N; lda = ldw = 3K).  splits: the forced K split (a workspace is registered when > 1).  auto: also run without a forced tile.
def _d(name, M, N, K, act=0, bias=1, resid=0, lda=None, ldw=None, ldc=None, ldr=None, vae=0, splits=1, cfgs=FORCED, auto=0, den=1, must_run=()):
    ldo = N // 2 if act == 2 else N
    lda, ldw = (3 * K, 3 * K) if vae else (lda or K, ldw or K)
    ldc = ldc or ldo
    ldr = ldc if resid == 2 else (ldr or N)
    return dict(name=name, kind="dense", M=M, N=N, K=K, act=act, bias=bias, resid=resid, lda=lda, ldw=ldw, ldc=ldc, ldr=ldr, vae=vae, splits=splits,
                cfgs=cfgs, auto=auto, den=den, must_run=tuple(x for x in FORCED if x in must_run))


def _c(name, B, Hin, Win, Cin, Cout, stride=1, pad=1, up=None, act=0, bias=1, resid=0, splits=1, cfgs=FORCED, auto=0, ws=0, must_run=()):
    Hup, Wup = up or (0, 0)
    return dict(name=name, kind="conv", B=B, Hin=Hin, Win=Win, Cin=Cin, Cout=Cout, stride=stride, pad=pad, Hup=Hup, Wup=Wup, act=act, bias=bias,
                resid=resid, splits=splits, cfgs=cfgs, auto=auto, ws=ws or splits > 1, den=1, must_run=tuple(x for x in FORCED if x in must_run))


V64 = (1, 2, 3, 4, 11, 5, 6, 7, 8, 9, 10)            # any N % 8 == 0: the LDS-DMA and 8-wave tiles, and the register-staged pair
REG = (9, 10)

DENSE = [
    # M around the tile heights x N around the tile widths x K = 1, 2, 3, 5, 11 K tiles; act 0 / 3, bias and residual on and off
    _d("m1_n64_k64", 1, 64, 64, must_run=V64),
    _d("m127_n128_k128_resid", 127, 128, 128, bias=0, resid=1, must_run=V64 + (15,)),
    _d("m129_n192_k192_relu", 129, 192, 192, act=3, resid=1, must_run=V64),
    _d("m255_n320_k320", 255, 320, 320, resid=1, must_run=V64 + (12, 14)),
    _d("m257_n640_k704_relu", 257, 640, 704, act=3, must_run=V64 + (14, 15)),
    _d("m513_n128_k64_bare", 513, 128, 64, bias=0, must_run=V64 + (15,)),
    _d("m300_n1280_k128", 300, 1280, 128, resid=1, must_run=V64 + (13, 14, 15)),
    # N % 8 != 0 or an odd ldc / ldr: the register-staged kernels alone
    _d("m300_n4_k64", 300, 4, 64, resid=1, auto=1, must_run=REG),
    _d("m129_n77_k192_relu_ldc77", 129, 77, 192, act=3, resid=1, auto=1, must_run=REG),
    _d("m129_n77_k192_ldc80", 129, 77, 192, ldc=80, auto=1, must_run=REG),
    _d("m257_n100_k320", 257, 100, 320, resid=1, auto=1, must_run=REG),
    _d("m127_n516_k128", 127, 516, 128, auto=1, must_run=REG),
    _d("m129_n128_k128_ldc129", 129, 128, 128, ldc=129, auto=1, must_run=REG),
    _d("m129_n128_k128_ldr133", 129, 128, 128, resid=1, ldr=133, auto=1, must_run=REG),
    # strided operands: padding columns are NaN, gap columns of C hold the sentinel
    _d("lda_k+8", 129, 128, 128, lda=136, must_run=V64 + (15,)),
    _d("ldw_k+64", 129, 128, 128, ldw=192, must_run=V64 + (15,)),
    _d("ldc_n+8", 129, 128, 128, resid=1, ldc=136, must_run=V64 + (15,)),
    _d("ldr_n+16", 129, 128, 128, resid=1, ldr=144, must_run=V64 + (15,)),
    _d("vae_qk_t77", 77, 77, 128, bias=0, vae=1, ldc=ceil64(77), auto=1, must_run=REG),
    _d("vae_qk_t200", 200, 200, 128, bias=0, vae=1, ldc=ceil64(200), must_run=V64),
    # in-place residual: N = 320 leaves the strip tile a partial last weight tile (forced cfg 12 must take the tiled kernel), N = 256 does not
    _d("inplace_n320_k320", 300, 320, 320, resid=2, auto=1, must_run=V64 + (12, 14)),
    _d("inplace_n256_k320", 300, 256, 320, resid=2, auto=1, must_run=V64 + (12, 13, 15)),
    _d("inplace_n640_k128_ldc648", 257, 640, 128, act=3, resid=2, ldc=648, auto=1, must_run=V64 + (14, 15)),
    # forced K splits: K = 704 is 22 steps of 32 -> 11 + 11, 8 + 8 + 6, 6 + 6 + 6 + 4; K = 256 is 8 steps, where the launcher caps 4 splits at 2
    _d("split2_k704", 257, 192, 704, resid=1, splits=2, cfgs=DMA, must_run=DMA),
    _d("split3_k704", 257, 192, 704, act=3, resid=1, splits=3, cfgs=DMA, must_run=DMA),
    _d("split4_k704", 257, 192, 704, splits=4, cfgs=DMA, must_run=DMA),
    _d("split4_k256", 129, 128, 256, resid=1, splits=4, cfgs=DMA, must_run=DMA),
]

CONV = [
    _c("s1p1_5x7_b3", 3, 5, 7, 64, 64, resid=1, must_run=V64),
    _c("s1p1_1x1_b1_relu", 1, 1, 1, 128, 128, act=3, must_run=V64 + (15,)),
    _c("s1p1_1x9_b3", 3, 1, 9, 64, 192, must_run=V64),
    _c("s1p1_9x1_b3", 3, 9, 1, 64, 320, resid=1, must_run=V64 + (14,)),
    _c("s2p1_7x9_b3", 3, 7, 9, 128, 64, stride=2, must_run=V64),
    _c("s2p1_8x10_b1", 1, 8, 10, 64, 640, stride=2, resid=1, must_run=V64 + (14, 15)),
    _c("s2p0_7x9_b3_relu", 3, 7, 9, 64, 128, stride=2, pad=0, act=3, resid=1, must_run=V64 + (15,)),
    _c("s2p0_8x10_b3", 3, 8, 10, 128, 320, stride=2, pad=0, must_run=V64 + (14,)),
    _c("up_6x5_11x9_b3", 3, 6, 5, 64, 320, up=(11, 9), resid=1, must_run=V64 + (14,)),
    _c("up_2x_5x4_b1", 1, 5, 4, 128, 128, up=(10, 8), must_run=V64 + (15,)),
    _c("up_w_only_3x6_b3", 3, 3, 6, 64, 640, up=(3, 12), must_run=V64 + (14, 15)),
    _c("up_h_only_6x3_b3_relu", 3, 6, 3, 64, 64, up=(12, 3), act=3, must_run=V64),
    _c("up_past_2x_3x3_7x5", 3, 3, 3, 64, 128, up=(7, 5), must_run=V64),              # Hup > 2 Hin: not for the 8-phase gather
    _c("up_6x5_11x9_b3_cout256", 3, 6, 5, 128, 256, up=(11, 9), act=3, resid=1, must_run=V64 + (13, 15)),      # the 8-phase 256x256 tile's gather
    _c("cin320_5x7_b3", 3, 5, 7, 320, 320, resid=1, must_run=V64 + (14,)),
    _c("cin320_s2p1_7x9_b3", 3, 7, 9, 320, 192, stride=2, must_run=V64),
    # small M, K = 2880: the automatic K split (with a workspace) and a forced uneven one (90 steps of 32 in 4 splits: 23 + 23 + 23 + 21)
    _c("cin320_splitk_auto", 1, 4, 4, 320, 128, resid=1, auto=1, ws=1, cfgs=(), must_run=()),
    _c("cin320_split4", 1, 4, 4, 320, 128, resid=1, splits=4, cfgs=DMA, must_run=DMA),
]

# non-linear epilogues on shapes of DENSE: an M tail, N = 640, an odd N; A and bias on the 1/8 lattice
_NL_SHAPES = [("m300_n320_k320", 300, 320, 320, V64 + (12, 14)), ("m129_n640_k128", 129, 640, 128, V64 + (14, 15)), ("m129_n77_k192", 129, 77, 192, REG)]
NONLIN = [_d(f"act{act}_{nm}", M, N, K, act=act, resid=1 if act == 5 else 0, den=8, auto=1 if N % 8 else 0, must_run=mr)
          for nm, M, N, K, mr in _NL_SHAPES for act in (1, 4, 5)]
# GEGLU: N counts the [value | gate] columns, the output has N / 2; no 320-wide tile, no residual
NONLIN += [_d("act2_m300_n640_k320", 300, 640, 320, act=2, den=8, must_run=(1, 2, 3, 4, 11, 7, 8, 12, 9)),
           _d("act2_m129_n1280_k128", 129, 1280, 128, act=2, den=8, must_run=(1, 2, 3, 4, 11, 7, 8, 13, 9))]

CASES = {c["name"]: c for c in DENSE + CONV + NONLIN}
assert len(CASES) == len(DENSE) + len(CONV) + len(NONLIN)

# nearest-index sweep: (n_in, n_up) for n_in in 1..24, n_up in n_in + 1 .. 2 n_in + 1; the other axis stays 4 wide.  One tile of each gather
# implementation: cfg 1 (csrc/gemm.hip), cfg 7 (csrc/gemm8.hip), cfg 15 (csrc/gemm8q.hip) -- the 8-phase tiles need Cout % 128 == 0 and take a scale
# of at most 2, so cfg 15 runs at C = 128 and on n_up <= 2 n_in.
SWEEP = [(i, u) for i in range(1, 25) for u in range(i + 1, 2 * i + 2)]
SWEEP_TILES = ((64, 1), (64, 7), (128, 15))            # (Cin = Cout, forced cfg)


def sweep_accepts(cfg, n_in, n_up):
    return cfg != 15 or n_up <= 2 * n_in


def make_dense(c):
    """-> dict(A, W, bias, resid): f16 CPU tensors of a dense case (W / bias of a GEGLU case in the [value | gate] order; None where absent)."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"]))
    M, N, K, den = c["M"], c["N"], c["K"], c["den"]
    if den == 1:
        A, W = lattice((M, K), INT_A, 0.2, seed), lattice((N, K), INT_W, 0.1, seed + 1)
        b = lattice((N,), INT_B, 0.0, seed + 2) if c["bias"] else None
        R = lattice((M, N), INT_B, 0.0, seed + 3) if c["resid"] else None
    else:
        # 1/8 lattice: |A| <= 1/2, a third of W non-zero -> z of a few units, where SiLU and GELU bend, and deep into both tails
        A, W = lattice((M, K), EIGHTHS, 0.2, seed), lattice((N, K), INT_W, 0.5, seed + 1)
        b = lattice((N,), tuple(v / 8 for v in range(-8, 9)), 0.0, seed + 2) if c["bias"] else None
        R = lattice((M, N), tuple(v / 8 for v in range(-8, 9)), 0.0, seed + 3) if c["resid"] else None
    # every partial sum of |products| stays far below 2^24 / den^2 (products of the 1/8 lattice are multiples of 1/8 as W is integer)
    assert K * float(A.abs().max()) * float(W.abs().max()) + 8 < 2.0 ** 24 / den
    return dict(A=A, W=W, bias=b, resid=R)


def make_conv(c):
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"]))
    B, Hin, Win, Cin, Cout = c["B"], c["Hin"], c["Win"], c["Cin"], c["Cout"]
    X, W = lattice((B, Hin, Win, Cin), INT_A, 0.2, seed), lattice((Cout, 9 * Cin), INT_W, 0.1, seed + 1)
    b = lattice((Cout,), INT_B, 0.0, seed + 2) if c["bias"] else None
    Ho, Wo = conv_out_hw(c["Hup"] or Hin, c["Wup"] or Win, c["stride"], c["pad"])
    R = lattice((B, Ho, Wo, Cout), INT_B, 0.0, seed + 3) if c["resid"] else None
    assert 9 * Cin * 2 + 8 < 2 ** 24
    return dict(X=X, W=W, bias=b, resid=R)


def reference(c, d):
    """-> (result, z, staged) of a case on its generated data."""
    if c["kind"] == "dense":
        return gemm_exact(d["A"], d["W"], d["bias"], d["resid"], c["act"], c["den"])
    return conv3x3_exact(d["X"], d["W"], d["bias"], d["resid"], c["stride"], c["pad"], c["Hup"], c["Wup"], c["act"], c["den"])


def plan_args(c):
    """The scalar arguments of tcl_gemm_plan / tcl_conv3x3_plan for a case (without the residual kind and the two outputs)."""
    if c["kind"] == "dense":
        return (c["M"], c["N"], c["K"], c["lda"], c["ldw"], c["ldc"], c["ldr"], c["act"])
    return (c["B"], c["Hin"], c["Win"], c["Cin"], c["Cout"], c["stride"], c["pad"], c["Hup"], c["Wup"], c["act"])
