"""References, case tables and tolerances of the leaf parity tests of csrc/elem.hip -- GroupNorm, LayerNorm, row softmax, GEGLU, GEMV, timestep
embedding, CFG unpack, AdaIN fusion, the SDE-DPM-Solver++ update (tests/test_gpu_elem_leaves.py; pinned on the CPU by tests/test_elem_refs_cpu.py).
torch on the CPU only.  Conventions and helpers are those of tests/leaf_refs.py.

Every `*_ref(..., dt)` evaluates one operation in the dtype `dt` on the kernel's own rounded inputs (f16 / f32 tensors, upcast) in the kernel's layout:
dt = float64 is the reference, dt = float32 the same operation at the precision the kernel accumulates in.  Scalars the C ABI takes as `float` are
rounded to float32 first, then upcast.

Tolerances
  exact      data movement / one rounding: torch.equal against the same IEEE sequence (yraw, untouched bytes, LayerNorm of a constant row).
  f16 output rel-L2 <= REL_F16 and |got - ref| <= 2^-10 |ref| + atol elementwise, atol = floor_atol(ref, inputs)[0] + 2^-24: the floor of
             leaf_refs.py plus one f16 subnormal step (softmax weights and saturated SiLU / GELU outputs land where the relative term is smaller than
             the rounding of the output itself).  The floor stays below ATOL_CAP of the output's RMS (test_elem_refs_cpu.py).
  f32 output (m0 of the DPM step) |got - ref| <= 2^-22 max(1, |ref|) elementwise: with p = fl(sigma_t eps), d = fl(x - p), q = fl(d / alpha_t) the error
             is at most 2^-24 (|p| / alpha_t + 2 |q|); the steps used have sigma_t / alpha_t <= 0.25, so |p| / alpha_t <= 1.25 for |eps| <= 5 and the sum
             is below 4 max(1, |q|) 2^-24, contracted multiply-add or not.

GroupNorm: the reference is the two-pass float64 GroupNorm of the concatenated input (groupnorm_two_pass_ref); the floor comes from groupnorm_ref, the
ONE-PASS form the kernel implements (mean = S1 / n, var = max(S2 / n - mean^2, 0)), so its float32-minus-float64 deviation is the cancellation floor
of the algorithm the kernel runs.  Inputs with an offset of 4 stay at HW <= 1024 and nothing goes above 4: at offset 8 the floor leaves the cap.
"""
import math

import torch
import torch.nn.functional as F

from leaf_refs import ATOL_CAP, REL_ELEM, REL_F16, elem_excess, floor_atol, is_sentinel16, rel_l2, rng, sentinel16  # noqa: F401  (re-exported)

F64, F32, H = torch.float64, torch.float32, torch.float16
SUB16 = 2.0 ** -24       # one f16 subnormal step
F32_REL = 2.0 ** -22     # the f32-output class


def f32s(v, dt):
    """A `float` argument of the C ABI: rounded to float32, then in dt."""
    return torch.tensor(float(v), dtype=F32).to(dt)


def group_excess(got, ref, atol, G):
    """Per-(sample, group) maximum of |got - ref| / (2^-10 |ref| + atol) for [B,HW,C] tensors -> [B,G]."""
    got, ref = got.to(F64), ref.to(F64)
    d, bound = (got - ref).abs(), REL_ELEM * ref.abs() + atol
    q = torch.where(d == 0, torch.zeros_like(d), d / bound)
    B, HW, C = q.shape
    return q.view(B, HW, G, C // G).amax(dim=(1, 3))


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
EPS_GN = 1e-5
GN_SHAPES = (  # B, HW, C1, C2, G
    (2, 37, 128, 0, 32),       # cpg 4: every chunk is two whole groups
    (2, 37, 192, 0, 32),       # cpg 6
    (1, 5, 224, 0, 32),        # cpg 7
    (3, 690, 320, 0, 32),      # cpg 10
    (2, 150, 328, 312, 32),    # cpg 20, the concat seam inside group 16
    (2, 150, 640, 320, 32),    # cpg 30
    (2, 70, 1280, 1280, 32),   # second channel window, group 25 across channel 2048, one row per block step
    (1, 33, 512, 0, 64),       # the largest G
    (1, 33, 64, 0, 1),         # one group
    (2, 2, 1280, 0, 32),       # the 1x2 mid block
    (1, 1, 320, 0, 32),        # a single row
    (1, 4099, 320, 320, 32),   # 65 stat blocks, the last with 3 rows
    (1, 16411, 128, 0, 32),    # the 256-block cap with a ragged tail; the 8-way interleave of k_gn_reduce fully used
)
GN_CASES = tuple((s, "std", 1) for s in GN_SHAPES) + (          # (shape, input kind, gamma scale)
    ((3, 690, 320, 0, 32), "off4", 1), ((2, 150, 640, 320, 32), "off4", 1),      # randn + 4: HW <= 1024 (module docstring)
    ((2, 150, 328, 312, 32), "std", 64))                                          # SiLU sees pre-activations beyond +-100
GN_REFUSED = (1, 9, 160, 0, 32)     # cpg 5: the chunk at channel 8 holds groups 1, 2 and 3


def gn_chunk_spans_three_groups(C, G):
    """The refusal rule of tcl_groupnorm_concat_f16, from the channel ranges themselves (not from the offset arithmetic of the library)."""
    cpg = C // G
    return any((8 * k + 7) // cpg - (8 * k) // cpg >= 2 for k in range(C // 8))


def gn_input(shape, kind, gscale):
    """-> x1 [B,HW,C1], x2 [B,HW,C2] or None, gamma [C], beta [C], all f16.  std: x1 = randn * 2 + 0.5, x2 = randn; off4: randn + 4 on both."""
    B, HW, C1, C2, G = shape
    g = rng(1000 * G + C1 + C2 + HW + (7 if kind == "off4" else 0) + gscale)
    if kind == "std":
        x1 = torch.randn(B, HW, C1, generator=g) * 2 + 0.5
        x2 = torch.randn(B, HW, C2, generator=g) if C2 else None
    else:
        x1 = torch.randn(B, HW, C1, generator=g) + 4
        x2 = torch.randn(B, HW, C2, generator=g) + 4 if C2 else None
    ga, be = torch.randn(C1 + C2, generator=g) * gscale, torch.randn(C1 + C2, generator=g)
    return x1.to(H), (x2.to(H) if C2 else None), ga.to(H), be.to(H)


def _gn_cat(x1, x2, G, dt):
    x = x1.to(dt) if x2 is None else torch.cat([x1.to(dt), x2.to(dt)], -1)
    B, HW, C = x.shape
    return x, x.view(B, HW, G, C // G)


def groupnorm_ref(x1, x2, gamma, beta, G, eps, silu, dt):
    """The one-pass form of k_gn_stats / k_gn_apply in dt: x1 [B,HW,C1] | x2 [B,HW,C2] -> [B,HW,C]."""
    x, xg = _gn_cat(x1, x2, G, dt)
    n = xg.shape[1] * xg.shape[3]
    mean = xg.sum(dim=(1, 3), keepdim=True) / n
    var = ((xg * xg).sum(dim=(1, 3), keepdim=True) / n - mean * mean).clamp_min(0)
    y = ((xg - mean) * torch.rsqrt(var + eps)).reshape(x.shape) * gamma.to(dt) + beta.to(dt)
    return F.silu(y) if silu else y


def groupnorm_two_pass_ref(x1, x2, gamma, beta, G, eps, silu, dt=F64):
    """torch.nn.GroupNorm (+ SiLU) with the variance taken about the mean."""
    x, xg = _gn_cat(x1, x2, G, dt)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape) * gamma.to(dt) + beta.to(dt)
    return F.silu(y) if silu else y


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
EPS_LN = 1e-5
LN_C = (8, 320, 512, 520, 640, 1280, 1544, 2048)      # NK 1..4; 520 and 1544: a chunk slot with one live lane
LN_ROWS = (1, 3, 4, 17, 999)                           # below / equal to / ragged against LN_R = 4, ragged against the 16 rows of a block
LN_CASES = tuple((C, rows, "std") for C in LN_C for rows in LN_ROWS) + ((640, 17, "off4"), (1544, 17, "const"))
LN_CONST_ROW, LN_CONST = 5, 1.5                        # row 5 of the "const" case holds 1.5 everywhere: f32 sums of it are exact, so y == beta exactly


def ln_input(C, rows, kind):
    g = rng(C * 7 + rows + len(kind))
    x = torch.randn(rows, C, generator=g) * 3
    if kind == "off4":
        x = x + 4
    if kind == "const":
        x[LN_CONST_ROW] = LN_CONST
    return x.to(H), torch.randn(C, generator=g).to(H), torch.randn(C, generator=g).to(H)


def layernorm_ref(x, gamma, beta, eps, dt):
    """x [rows,C]: mean, variance about the mean (the kernel's two passes over the row in registers)."""
    x = x.to(dt)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * gamma.to(dt) + beta.to(dt)


# ------------------------------------------------------------------------------------------------------------------ row softmax
SOFTMAX_SCALE, SOFTMAX_ROWS = 0.3, 3
SOFTMAX_CASES = (  # T, ld, form
    (8, 8, "reg"), (1000, 1000, "reg"), (2048, 2048, "reg"), (2056, 2056, "reg"), (16384, 16384, "reg"),     # 2056: first chunk of the second slot; 16384: all eight
    (1000, 1008, "reg"), (2056, 2064, "reg"),                                                                   # ld = T + 8
    (1, 1, "lds"), (7, 7, "lds"), (1001, 1001, "lds"), (16392, 16392, "lds"),
    (1000, 1004, "lds"),                                                                                        # T % 8 == 0 but ld % 8 != 0
    (7, 15, "lds"), (1001, 1009, "lds"))                                                                        # ld = T + 8
SOFTMAX_KINDS = ("noise", "spike", "equal", "min")      # one kind per run: the floor of a run is a single figure, taken over rows of one character


def softmax_kinds(T):
    """The spike rows stay at T <= 2056: behind a weight of 1 a float32 sum drops most of 16 383 further weights of 1e-7 and below, and the floor of
    such a run (2.2e-5 at T = 16384 against an output RMS of 7.8e-3) leaves ATOL_CAP -- the rule that keeps GroupNorm's offset 4 at HW <= 1024."""
    return tuple(k for k in SOFTMAX_KINDS if k != "spike" or T <= 2056)


def softmax_form(T, ld):
    """The dispatch rule of tcl_softmax_rows_f16."""
    return "reg" if T % 8 == 0 and ld % 8 == 0 and T <= 16384 else "lds"


def softmax_input(T, kind):
    """[3,T] f16.  noise: randn * 4.  spike: randn * 4 with one entry 40 above the row's maximum (every other weight rounds to 0 or an f16 subnormal), at
    column 5T/7, 0 and T - 1.  equal: a constant row (every weight 1 / T).  min: randn * 4 with one entry -65504."""
    g = rng(T + 50000 * SOFTMAX_KINDS.index(kind))
    x = torch.randn(SOFTMAX_ROWS, T, generator=g) * 4
    for r, col in enumerate(((T * 5) // 7, 0, T - 1)):
        if kind == "spike":
            x[r, col] = x[r].max() + 40
        elif kind == "min":
            x[r, col] = -65504.0
    if kind == "equal":
        x[:] = torch.tensor([2.5, -7.0, 0.0])[:, None]
    return x.to(H)


def softmax_ref(x, scale, dt):
    return torch.softmax(x.to(dt) * f32s(scale, dt), -1)


# ------------------------------------------------------------------------------------------------------------------ GEGLU / GEMV / timestep embedding
GEGLU_CASES = tuple((D, rows) for D in (8, 1280) for rows in (1, 500))


def geglu_input(D, rows):
    """[rows, 2D] f16 = [value | gate]; gates randn * 3, row 0 sweeps -12 .. 12 (both saturated tails of erff)."""
    x = torch.randn(rows, 2 * D, generator=rng(D + rows))
    x[:, D:] *= 3
    x[0, D:] = torch.linspace(-12, 12, D)
    return x.to(H)


def geglu_ref(x, dt):
    D = x.shape[1] // 2
    return x[:, :D].to(dt) * F.gelu(x[:, D:].to(dt))


GEMV_SHAPES = ((1280, 320), (1280, 1280), (6, 8), (321, 520))       # N, K: N not a multiple of 4, K ragged against the 512-element lane stride
GEMV_FLAGS = (  # silu_in, silu_out, bias, add: the three calls of UNetEngine._temb, and the bare product
    (0, 1, True, False), (0, 0, True, False), (1, 0, True, True), (0, 0, False, False))
GEMV_CASES = tuple((N, K, fl) for N, K in GEMV_SHAPES for fl in GEMV_FLAGS)


def _f16_ambiguous(v64, margin):
    """Where the f16 rounding of float64 values is within `margin` (relative to the f16 spacing there) of a tie."""
    r = v64.to(H).to(F64)
    ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -14))) - 10), torch.tensor(SUB16, dtype=F64))
    return ((v64 - r).abs() / ulp - 0.5).abs() < margin


def gemv_input(N, K, flags):
    """W [N,K], x [K], bias [N], add [N] f16.  With silu_in the kernel rounds SiLU(x) to f16: entries of x whose SiLU lies within 2^-8 of an f16 spacing
    of a rounding tie are moved to the next f16 value, so the float32 and the float64 SiLU round alike and the reference has ONE vector to multiply."""
    g = rng(N * 3 + K + sum(int(f) << i for i, f in enumerate(flags)))
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(H)
    x = torch.randn(K, generator=g).to(H)
    if flags[0]:
        for _ in range(8):
            amb = _f16_ambiguous(F.silu(x.to(F64)), 2.0 ** -8)
            if not amb.any():
                break
            x = torch.where(amb, (x.view(torch.int16) + 1).view(H), x)
        assert not _f16_ambiguous(F.silu(x.to(F64)), 2.0 ** -8).any()
    return W, x, torch.randn(N, generator=g).to(H), torch.randn(N, generator=g).to(H)


def gemv_presum_ref(W, x, bias, silu_in, silu_out, dt):
    """act(W . f16(silu(x)) + bias): the value the kernel rounds to f16 (and, without `add`, stores)."""
    xv = x.to(dt)
    if silu_in:
        xv = F.silu(xv).to(H).to(dt)
    s = W.to(dt) @ xv
    if bias is not None:
        s = s + bias.to(dt)
    return F.silu(s) if silu_out else s


def gemv_ref(W, x, bias, add, silu_in, silu_out, dt):
    s = gemv_presum_ref(W, x, bias, silu_in, silu_out, dt)
    return s if add is None else s.to(H).to(dt) + add.to(dt)


def gemv_alt_ref(W, x, bias, add, silu_in, silu_out, presum_atol):
    """With `add` the sum is rounded to f16 BEFORE the addition.  Where the float64 sum lies within presum_atol of a rounding tie, the float32 sum of the
    kernel may round to the other neighbour: -> (ambiguous mask [N], the reference with that neighbour).  Both are float64."""
    s = gemv_presum_ref(W, x, bias, silu_in, silu_out, F64)
    r = s.to(H)
    away = s.abs() > r.to(F64).abs()
    other = (r.view(torch.int16) + torch.where(away, 1, -1).to(torch.int16)).view(H)
    other = torch.where(r == 0, r, other).to(F64)
    amb = ((s - 0.5 * (r.to(F64) + other)).abs() <= presum_atol) & (other != r.to(F64))
    return amb, other + add.to(F64)


TEMB_DIM, TEMB_T = 320, (0.0, 1.0, 21.0, 601.0, 999.0)


def timestep_embed_ref(t, dim, dt):
    """diffusers Timesteps(flip_sin_to_cos=True, freq_shift=0): [cos | sin]."""
    half = dim // 2
    freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dt) / half)
    a = f32s(t, dt) * freq
    return torch.cat([torch.cos(a), torch.sin(a)])


# ------------------------------------------------------------------------------------------------------------------ sampler glue
UNPACK_N, UNPACK_H, UNPACK_W = 7, 5, 7
UNPACK_CASES = (  # name, mode, idx, sl, nwin, guidance, scale_upto, scale, nkeep
    ("xy", 0, (5, 1, 2), 0, 0, 1.75, 0, 1.0, 0),
    ("yt", 1, (6, 0, 4, 2), 2, 4, 1.75, 3, math.sqrt(0.5), 2))      # columns neither sorted nor contiguous; nkeep < nwin; scale_upto inside the window


def unpack_input(case):
    name, mode, idx, sl, nwin = case[:5]
    Hh, Ww = (nwin, UNPACK_H) if mode else (UNPACK_H, UNPACK_W)
    return torch.randn(2 * len(idx), Hh, Ww, 4, generator=rng(31 + mode)).to(H)


def unpack_cfg_ref(eps, case, dt):
    """eps [2F,Hh,Ww,4] -> (noise [N,4,h,w] in dt, zero where nothing is written; written mask [N,4,h,w])."""
    name, mode, idx, sl, nwin, guidance, scale_upto, scale, nkeep = case
    Fn, h, w = len(idx), UNPACK_H, UNPACK_W
    e = eps.to(dt)
    pred = e[:Fn] + f32s(guidance, dt) * (e[Fn:] - e[:Fn])         # [F,Hh,Ww,4]
    out, mask = torch.zeros(UNPACK_N, 4, h, w, dtype=dt), torch.zeros(UNPACK_N, 4, h, w, dtype=torch.bool)
    for j, ix in enumerate(idx):
        if mode == 0:
            out[ix], mask[ix] = pred[j].permute(2, 0, 1), True                      # frame ix: [h,w,4] -> [4,h,w]
        else:
            for yy in range(min(nkeep, nwin)):                                      # frame sl + yy, column ix: [h,4] -> [4,h]
                n = sl + yy
                out[n, :, :, ix] = pred[j, yy].t() * (f32s(scale, dt) if n < scale_upto else 1.0)
                mask[n, :, :, ix] = True
    return out, mask


def unpack_cfg_values_ref(eps, case, dt):
    return unpack_cfg_ref(eps, case, dt)[0]


ADAIN_HW, ADAIN_PLANES, ADAIN_ALPHA = (2, 120, 257), 5, 0.01


def adain_input(hw):
    """nt, nxy [planes, hw] f16, mean 3 / std 0.2 (nxy: mean -3 on odd planes, std 0.4)."""
    g = rng(hw)
    a = 3 + 0.2 * torch.randn(ADAIN_PLANES, hw, generator=g)
    b = 3 + 0.4 * torch.randn(ADAIN_PLANES, hw, generator=g)
    b[1::2] -= 6
    return a.to(H), b.to(H)


def adain_first_ref(a, b, dt):
    """adaptive_instance_normalization(nt, nxy): unbiased variance, eps 1e-5 inside the root."""
    a, b = a.to(dt), b.to(dt)
    sa, sb = torch.sqrt(a.var(-1, keepdim=True) + 1e-5), torch.sqrt(b.var(-1, keepdim=True) + 1e-5)
    return (a - a.mean(-1, keepdim=True)) / sa * sb + b.mean(-1, keepdim=True)


def adain_second_ref(a_rounded, b, alpha, dt):
    """sqrt(alpha) * f16(AdaIN) + sqrt(1 - alpha) * nxy -- from the ROUNDED first output, as the kernel does."""
    al = f32s(alpha, dt)
    return torch.sqrt(al) * a_rounded.to(dt) + torch.sqrt(1 - al) * b.to(dt)


def adain_second_from_inputs_ref(a, b, alpha, dt):
    return adain_second_ref(adain_first_ref(a, b, F64).to(H), b, alpha, dt)


DPM_STEPS, DPM_BEGIN = 20, 15       # the 20-step schedule entered at index 15 (img2img): step 15 first order, step 16 second order; sigma 0.23 and 0.14
DPM_N = (1, 1003)
DPM_CASES = tuple((n, second, with_z) for n in DPM_N for second in (False, True) for with_z in (False, True))


def dpm_coefficients(second):
    """(sigma_t, alpha_t, ca, cb0, cb1, cc) of tc_light_amd.scheduler for the first (order 1) / second (order 2) executed step."""
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    sch = DPMSolverSDEScheduler()
    sch.set_timesteps(DPM_STEPS, begin=DPM_BEGIN)
    return sch.coefficients(DPM_BEGIN + (1 if second else 0), second)


def dpm_input(n, second, with_z):
    """x, eps, z f16 [n]; m1 f32 [n] (the previous step's x0)."""
    g = rng(n + 2 * second + with_z)
    x, eps, z = (torch.randn(n, generator=g).to(H) for _ in range(3))
    return x, eps, (torch.randn(n, generator=g) if second else None), (z if with_z else None)


def dpm_m0_ref(x, eps, coef, dt):
    sigma_t, alpha_t = coef[:2]
    return (x.to(dt) - f32s(sigma_t, dt) * eps.to(dt)) / f32s(alpha_t, dt)


def dpm_x_ref(x, eps, m1, z, coef, dt):
    _, _, ca, cb0, cb1, cc = coef
    r = f32s(ca, dt) * x.to(dt) + f32s(cb0, dt) * dpm_m0_ref(x, eps, coef, dt)
    if m1 is not None:
        r = r + f32s(cb1, dt) * m1.to(dt)
    return r if z is None else r + f32s(cc, dt) * z.to(dt)


# ------------------------------------------------------------------------------------------------------------------ the f16-class cases and their floors
def f16_floor_cases():
    """Every (kernel, case id, ref_fn, args) of the f16-output class: what test_elem_refs_cpu.py caps and the GPU tests take their atol from."""
    for shape, kind, gscale in GN_CASES:
        x1, x2, ga, be = gn_input(shape, kind, gscale)
        for silu in (0, 1):
            yield "groupnorm", (shape, kind, gscale, silu), groupnorm_ref, (x1, x2, ga, be, shape[4], EPS_GN, silu)
    for C, rows, kind in LN_CASES:
        yield "layernorm", (C, rows, kind), layernorm_ref, (*ln_input(C, rows, kind), EPS_LN)
    for T, ld, form in SOFTMAX_CASES:
        for kind in softmax_kinds(T):
            yield "softmax_rows", (T, ld, kind), softmax_ref, (softmax_input(T, kind), SOFTMAX_SCALE)
    for D, rows in GEGLU_CASES:
        yield "geglu", (D, rows), geglu_ref, (geglu_input(D, rows),)
    for N, K, fl in GEMV_CASES:
        W, x, b, a = gemv_input(N, K, fl)
        yield "gemv", (N, K, fl), gemv_ref, (W, x, b if fl[2] else None, a if fl[3] else None, fl[0], fl[1])
        if fl[3]:
            yield "gemv_presum", (N, K, fl), gemv_presum_ref, (W, x, b if fl[2] else None, fl[0], fl[1])
    for t in TEMB_T:
        yield "timestep_embed", (t,), timestep_embed_ref, (t, TEMB_DIM)
    for case in UNPACK_CASES:
        yield "unpack_cfg", (case[0],), unpack_cfg_values_ref, (unpack_input(case), case)
    for hw in ADAIN_HW:
        a, b = adain_input(hw)
        yield "adain_first", (hw,), adain_first_ref, (a, b)
        yield "adain_second", (hw,), adain_second_from_inputs_ref, (a, b, ADAIN_ALPHA)
    for n, second, with_z in DPM_CASES:
        x, eps, m1, z = dpm_input(n, second, with_z)
        yield "dpm_step_x", (n, second, with_z), dpm_x_ref, (x, eps, m1, z, dpm_coefficients(second))


_ATOL = {}


def atol_of(kernel, case):
    """floor_atol of one case of f16_floor_cases(), cached: -> (floor, rms).  The elementwise atol of the GPU tests is floor + SUB16."""
    if not _ATOL:
        for name, cid, fn, args in f16_floor_cases():
            _ATOL[(name, cid)] = (fn, args)
    v = _ATOL[(kernel, tuple(case))]
    if callable(v[0]):
        v = _ATOL[(kernel, tuple(case))] = floor_atol(v[0], *v[1])
    return v
