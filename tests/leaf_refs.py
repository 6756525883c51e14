"""References and tolerances of the leaf parity tests of the producer and VAE glue kernels (tests/test_gpu_producer_leaves.py; pinned on the CPU by
tests/test_leaf_refs_cpu.py).  torch on the CPU only.

Every `*_ref(..., dt)` evaluates one operation in the dtype `dt` on the kernel's own rounded inputs (f16 or f32 tensors, upcast): dt = float64 is the
reference, dt = float32 the same operation at the precision the kernels accumulate in.  Where oracle/ states the operation it is called with the
upcast tensors.  Layouts are the kernels' (NHWC rows, tap-major weights), so the helpers also pin the index conventions of include/tclight_hip.h.

Tolerances
  exact      data movement / one rounding: the test restates the IEEE sequence in torch and asserts torch.equal.
  f16 output rel-L2 <= REL_F16 and |got - ref| <= 2^-10 |ref| + atol elementwise, atol = floor_atol(ref, inputs) = 4 x the largest deviation of the
             float32 evaluation from the float64 one on the same inputs (4: another summation order), capped at ATOL_CAP of the output's RMS.
  f32 output |got - ref| <= F32_ABS * max(1, max|ref|)  (the f32 figure of tests/test_gpu_memflow.py).
"""
import torch
import torch.nn.functional as F

from oracle import memflow as OM
from oracle import rmbg as OR

F64, F32, H = torch.float64, torch.float32, torch.float16
REL_F16 = 2e-3          # per-op rel-L2 of an f16-output kernel (tests/test_gpu_kernels.py)
REL_ELEM = 2.0 ** -10   # one f16 ulp, relative: twice the rounding of the output
ATOL_CAP = 2e-3         # floor_atol must stay below this fraction of the output's RMS
F32_ABS = 3e-5          # f32 kernels, values of order 1 (tests/test_gpu_memflow.py)
SENT16 = 0x7DEF         # f16 sentinel bit pattern (a NaN: reading it poisons the output, and a bit compare still sees it)


def rng(seed):
    return torch.Generator().manual_seed(seed)


def sentinel16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16).view(H)


def is_sentinel16(t):
    return bool((t.contiguous().view(torch.int16) == SENT16).all())


def rel_l2(got, ref):
    got, ref = got.to(F64), ref.to(F64)
    return ((got - ref).norm() / ref.norm().clamp_min(1e-12)).item()


def floor_atol(ref_fn, *args):
    """-> (atol, rms): atol = 4 * max |ref_fn(dt=float32) - ref_fn(dt=float64)|, rms of the float64 output."""
    r64 = ref_fn(*args, dt=F64)
    r32 = ref_fn(*args, dt=F32).to(F64)
    return 4.0 * (r32 - r64).abs().max().item(), r64.pow(2).mean().sqrt().item()


def elem_excess(got, ref, atol):
    """Largest |got - ref| / (2^-10 |ref| + atol) (<= 1 passes); 0 / 0 counts as 0."""
    got, ref = got.to(F64), ref.to(F64)
    d, bound = (got - ref).abs(), REL_ELEM * ref.abs() + atol
    q = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return q.max().item()


def f32_tol(ref, magnitude=None):
    return F32_ABS * max(1.0, float(ref.abs().max()) if magnitude is None else float(magnitude))


# ------------------------------------------------------------------------------------------------------------------ MemFlowNet / RAFT encoders
def stem_weight_t(w):
    """[64,3,7,7] -> w_t [147,64] with row c*49 + ky*7 + kx."""
    return w.reshape(64, 147).t().contiguous()


def conv7x7s2_ref(x, w, bias, relu, dt):
    """x [B,3,H,W], w [64,3,7,7] -> NHWC [B,Ho,Wo,64]."""
    y = F.conv2d(x.to(dt), w.to(dt), bias.to(dt), stride=2, padding=3)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()


def instnorm_nchw(x, eps):
    """InstanceNorm2d, affine=False, biased variance; any number of spatial elements (F.instance_norm refuses a single one)."""
    m = x.mean(dim=(2, 3), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(2, 3), keepdim=True)
    return (x - m) / torch.sqrt(v + eps)


def conv7x7s2_instnorm_ref(x, w, bias, eps, dt):
    y = F.conv2d(x.to(dt), w.to(dt), bias.to(dt), stride=2, padding=3)
    return F.relu(instnorm_nchw(y, eps)).permute(0, 2, 3, 1).contiguous()


def instnorm_ref(x, eps, relu, dt):
    """x [B,HW,C] rows -> [B,HW,C]."""
    y = instnorm_nchw(x.to(dt).permute(0, 2, 1)[..., None], eps)[..., 0].permute(0, 2, 1)
    return (F.relu(y) if relu else y).contiguous()


def instnorm_input(B, HW, C, seed):
    """Rows [B,HW,C] f16: channel 1 all zero (the 96 -> 128 channel padding of EncoderEngine), channel 2 mean 6 / std 0.05 (a one-pass f32 variance
    loses its digits there), the others N(offset, scale) with per-channel offset and scale."""
    g = rng(seed)
    x = torch.randn(B, HW, C, generator=g) * (0.25 + 2 * torch.rand(1, 1, C, generator=g)) + torch.randn(1, 1, C, generator=g)
    x[..., 1] = 0
    x[..., 2] = 6 + 0.05 * torch.randn(B, HW, generator=g)
    return x.to(H)


def add_act_ref(a, b, act, dt):
    t = a.to(dt) + b.to(dt)
    return F.relu(t) if act == 3 else F.gelu(t) if act == 4 else t


GELU_EDGES = (0.0, -0.0, 10.0, -10.0, 1e-3, -1e-3, 3.0, -3.0)


def tanh_ref(x, dt):
    return torch.tanh(x.to(dt))


# ------------------------------------------------------------------------------------------------------------------ update block
def dw_weight_conv(w, k):
    """tap-major [k*k, C] -> Conv2d(groups=C) weight [C,1,k,k]."""
    return w.t().reshape(w.shape[1], 1, k, k)


def dwconv_gelu_ref(x, w, bias, k, dt):
    """x [B,H,W,C] NHWC, w [k*k,C], bias [C] -> gelu(x + depthwise(x) + bias), NHWC."""
    xn = x.to(dt).permute(0, 3, 1, 2)
    y = F.gelu(xn + F.conv2d(xn, dw_weight_conv(w.to(dt), k), bias.to(dt), padding=k // 2, groups=xn.shape[1]))
    return y.permute(0, 2, 3, 1).contiguous()


def upsample_flow_ref(flow, mask_rows, mask_scale, dt):
    """flow [B,2,h,w], mask rows [B*h*w, >=576] (channel tap*64 + i*8 + j) -> oracle.memflow.upsample_flow on the scaled mask."""
    B, _, h, w = flow.shape
    m = mask_rows[:, :576].to(dt).view(B, h, w, 576).permute(0, 3, 1, 2).contiguous() * mask_scale
    return OM.upsample_flow(flow.to(dt), m)


def avgpool2_nhwc_ref(x, dt):
    return F.avg_pool2d(x.to(dt).permute(0, 3, 1, 2), 2, stride=2).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ BriaRMBG
def conv3x3_weight_t(w):
    """[Cout,Cin,3,3] -> w_t [Cin*9, Cout], tap index ky*3 + kx."""
    return w.reshape(w.shape[0], -1).t().contiguous()


def conv3x3_direct_ref(x1, x2, w, scale, shift, resid, dil, stride, relu, dt):
    x = x1.to(dt) if x2 is None else torch.cat([x1.to(dt), x2.to(dt)], 1)
    y = F.conv2d(x, w.to(dt), None, stride=stride, padding=dil, dilation=dil) * scale.to(dt)[None, :, None, None] + shift.to(dt)[None, :, None, None]
    if relu:
        y = F.relu(y)
    return y if resid is None else y + resid.to(dt)


def fold_bn(bias, mean, var, gamma, beta, eps=1e-5):
    """eval BatchNorm + conv bias as the kernel's per-channel (scale, shift)."""
    s = gamma / torch.sqrt(var + eps)
    return s, beta + (bias - mean) * s


def maxpool2_ceil_ref(x, dt):
    return OR._pool(x.to(dt))


def resize_bilinear_ref(x, Ho, Wo, mul, sigmoid, clamp01, dt):
    y = OR._up(x.to(dt), torch.empty(1, 1, Ho, Wo)) * mul
    if sigmoid:
        y = torch.sigmoid(y)
    return y.clamp(0, 1) if clamp01 else y


# ------------------------------------------------------------------------------------------------------------------ VAE glue
def conv1x1_small_ref(x, W, b, dt):
    """x [M,Ci], W [Co,Ci], b [Co] -> [M,Co]."""
    return x.to(dt) @ W.to(dt).t() + b.to(dt)


def im2col3x3_ref(x, Kpad):
    """x [B,H,W,Cin] -> [B*H*W, Kpad], column tap*Cin + c (tap = ky*3 + kx, padding 1), zeros from 9*Cin on."""
    B, Hh, Ww, C = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
    taps = [xp[:, :, ky:ky + Hh, kx:kx + Ww].permute(0, 2, 3, 1) for ky in range(3) for kx in range(3)]
    out = torch.zeros(B * Hh * Ww, Kpad, dtype=x.dtype)
    out[:, :9 * C] = torch.stack(taps, 3).reshape(B * Hh * Ww, 9 * C)
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases of the f16-output kernels
STEM_SIZES = ((37, 53), (16, 24), (7, 5))        # Ho*Wo = 513 (ragged third block of 256) / one block / every window clipped
INSTNORM_C, INSTNORM_HW, INSTNORM_B = (8, 64, 128, 256), (1, 63, 257, 4099), (1, 3)
DW_K, DW_C = (1, 7, 15), (8, 24)
DW_SIZES = ((5, 3), (16, 16), (17, 33), (24, 40))  # all halo / one tile / tile tails on both axes / several tiles
CONV1X1 = ((4, 4, 8, 8), (8, 8, 8, 64), (8, 8, 512, 8))     # Ci, Co, ldi, ldo
CONV3X3 = (  # C1, C2, Cout, dil, stride, relu, resid, H, W
    (3, 0, 64, 1, 2, 1, False, 13, 17), (16, 16, 16, 1, 1, 1, True, 15, 20), (8, 0, 1, 1, 1, 0, False, 9, 11),
    (8, 0, 24, 2, 1, 1, False, 9, 11), (16, 0, 16, 4, 1, 1, False, 9, 11), (16, 16, 16, 8, 1, 1, True, 5, 7))
RESIZE = ((5, 7, 10, 14), (5, 7, 9, 13), (30, 50, 64, 64), (64, 64, 30, 50), (1, 1, 4, 4))


def stem_input(Hh, Ww, seed, unit_range):
    g = rng(seed)
    x = torch.rand(2, 3, Hh, Ww, generator=g) if unit_range else torch.randn(2, 3, Hh, Ww, generator=g)
    return x, torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5, torch.randn(64, generator=g) * 0.5


def dwconv_input(k, C, Hh, Ww, seed):
    g = rng(seed)
    x = torch.randn(2, Hh, Ww, C, generator=g).to(H)
    return x, (torch.randn(k * k, C, generator=g) / k).to(H), torch.randn(C, generator=g).to(H)


def add_act_input(n, seed):
    g = rng(seed)
    a, b = torch.randn(n, generator=g).to(H), torch.randn(n, generator=g).to(H)
    a[:8] = torch.tensor(GELU_EDGES).to(H)
    b[:8] = 0
    b[1] = -0.0
    return a, b


def context_input(P, seed):
    c = (torch.randn(P, 256, generator=rng(seed)) * 3).clamp(-9, 9).to(H)
    c[0, :4] = torch.tensor([9.0, -9.0, 0.0, -0.0]).to(H)
    c[0, 128:132] = torch.tensor([9.0, -9.0, 0.0, -0.0]).to(H)
    return c


def conv1x1_input(Ci, Co, M, seed):
    g = rng(seed)
    return torch.randn(M, Ci, generator=g).to(H), (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).to(H), torch.randn(Co, generator=g).to(H)


def f16_floor_cases():
    """Every (kernel, case id, ref_fn, args) of the f16-output class: what test_leaf_refs_cpu.py pins and the GPU tests take their atol from."""
    for Hh, Ww in STEM_SIZES:
        for relu in (0, 1):
            x, w, b = stem_input(Hh, Ww, Hh, False)
            yield "conv7x7s2_c3", (Hh, Ww, relu), conv7x7s2_ref, (x, w, b, relu)
        x, w, b = stem_input(Hh, Ww, Hh + 1, True)
        yield "conv7x7s2_instnorm", (Hh, Ww), conv7x7s2_instnorm_ref, (x, w, b, 1e-5)
    for C in INSTNORM_C:
        for HW in INSTNORM_HW:
            for B in INSTNORM_B:
                yield "instnorm", (C, HW, B), instnorm_ref, (instnorm_input(B, HW, C, C + HW + B), 1e-5, 0)
    for k in DW_K:
        for C in DW_C:
            for Hh, Ww in DW_SIZES:
                yield "dwconv_gelu", (k, C, Hh, Ww), dwconv_gelu_ref, (*dwconv_input(k, C, Hh, Ww, k + C + Hh), k)
    for n in (8, 8 * 1025 + 8):
        yield "add_act_gelu", (n,), add_act_ref, (*add_act_input(n, n), 4)
    for P in (1, 257):
        yield "context_split_tanh", (P,), tanh_ref, (context_input(P, P)[:, :128],)
    for Ci, Co, ldi, ldo in CONV1X1:
        for M in (1, 1000):
            yield "conv1x1_small", (Ci, Co, ldi, ldo, M), conv1x1_small_ref, conv1x1_input(Ci, Co, M, Ci + Co + ldi + M)


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
