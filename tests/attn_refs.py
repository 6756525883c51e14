"""References, case table, inputs and the elementwise bound of the leaf parity tests of csrc/attn.hip -- the flash kernels of every head dim, the gated
exact pass behind the speculative d = 40 kernel, split-KV (tests/test_gpu_attn_leaves.py; pinned on the CPU by tests/test_attn_refs_cpu.py).  torch on
the CPU only.  Conventions and helpers are those of tests/leaf_refs.py.

Tensors are [B, T, H, d] f16 (q) and [Bkv, Tk, H, d] f16 (k, v); kv_map[b] is the K / V entry of sample b.

attention_ref(q, k, v, scale, kv_map, dt) works on the kernel's own rounded inputs: Qs = f16(f32(q) * f32(f32(scale) * f32(log2 e))) exactly as
pack_rows_blk does it, then Qs.K^T, a base-2 softmax and P.V in dt (float64: the reference; float32: the floor).  It also returns A = softmax(S).|V|.

flash_emulated(..., off) is the arithmetic the kernels run -- f32 scores, a shift m = f16(rowmax + off) (off = 0: the exact kernels, 3: the speculative
one), P = f16(exp2(s - m)), f32 sums of P.V and of P, one division, an f16 store; with nsplit > 1 every chunk's normalised output is rounded to f16 and
the chunks are joined in f32 from log2 of their denominators (k_flash_lse / k_attn_merge).  It only pins the bound on the CPU.

Elementwise bound (from the arithmetic, not from a GPU run)
    |got - ref| <= 2^-10 |ref| + cA A + Tk 2^-22 max|v| + atol,   cA = 2^-10 (2^-10 + 2^-11 for split-KV),   atol = 4 max|ref_f32 - ref_f64| + 2^-24
  every P carries a relative rounding of 2^-11: <= 2^-11 A in the numerator and <= 2^-11 |ref| through the denominator; the output rounding is 2^-11 |ref|;
  a P in the f16 subnormal range has an absolute error of 2^-25 against a largest P of the row >= 2^-3 (speculative kernel; larger in the others), which
  after the normalisation is at most 2^-22 max|v| per key; split-KV rounds each chunk's partial output once more (2^-11 A).

Input kinds (seeded per case and sample: sample b of a case is randn(max(Tq, Tk), 3 H d) from the seed case.seed * 4096 + b, columns [q | k | v])
  noise               as drawn
  peaked              q x 6: logit std about 9 bits
  last_key            for one row per spiked sample, key Tk - 1 is 4 x that row of q: the row's output is about v[Tk - 1]
  first_of_last_tile  the same at key 64 (ceil(Tk / 64) - 1)
  v_ones              V = 1: every output element is within one rounding of 1.  K carries a common offset u and rows 0 and Tq - 1 of every sample are
                      -1.5 u, so every valid key of those rows scores 14 .. 27 bits BELOW zero: a padded key (score 0) that is counted swamps the row sum
  overflow            test_gated_exact_pass_small alone: see overflow_spikes
"""
import functools
from collections import namedtuple

import torch

from leaf_refs import ATOL_CAP, REL_ELEM, SENT16, is_sentinel16, rel_l2, rng, sentinel16  # noqa: F401  (re-exported)

F64, F32, H = torch.float64, torch.float32, torch.float16
SUB16 = 2.0 ** -24       # one f16 subnormal step
LOG2E = 1.4426950408889634
KV_TILE = 64
# the ids tcl_attention_plan reports (csrc/attn.hip: the rows of g_flash)
FV_40_SPEC, FV_40_QB2, FV_40_QB1, FV_80, FV_128, FV_160 = range(6)
FV_NAMES = ("d40 speculative", "d40 qb2 exact", "d40 qb1", "d80", "d128", "d160")
SPLITKV = 6              # not a row of g_flash: k_flash_lse + k_attn_merge (named here for the records only)

KINDS = ("noise", "peaked", "last_key", "first_of_last_tile", "v_ones")
SPIKED = ("last_key", "first_of_last_tile")
SPLIT_KINDS = ("noise", "last_key", "v_ones")     # last_key: the spike is in the last chunk, which then dominates the merge
SPIKE_GAIN, PEAK_GAIN, ANTI_GAIN = 4.0, 6.0, -1.5

# layout: "qkv" = Q, K, V are column slices of one fused [B, T, 3C] tensor (ld = 3C); "kv" = Q dense, K | V slices of a fused [Bkv, Tk, 2C] tensor (ld = 2C);
# "ld256" = the MemFlowNet read: q the first 128 columns of a [Tq, 256] tensor, K | V a [Tk, 256] tensor
Case = namedtuple("Case", "variant d B H Tq Tk kv_div layout nsplit seed")


def _case(variant, d, B, H, Tq, Tk, kv_div=1, layout=None, nsplit=1):
    layout = layout or ("ld256" if d == 128 else "kv" if kv_div > 1 else "qkv")
    return Case(variant, d, B, H, Tq, Tk, kv_div, layout, nsplit, (variant * 37 + d + 3 * B + 5 * H + 7 * Tq + 11 * Tk + 13 * kv_div + 17 * nsplit) % 100003)


CASES = tuple(
    # d = 40, one query block per wave (B H ceil(Tq / 256) < 1024): every Tk once, every Tq twice
    [_case(FV_40_QB1, 40, 2, 8, Tq, Tk) for Tq, Tk in ((1, 1), (127, 2), (128, 63), (129, 64), (300, 65), (1, 127), (127, 128), (128, 129), (129, 192), (300, 321))]
    # d = 40 speculative (B H ceil(Tq / 256) >= 1024; TPB = 2): (nfull, nt) = (0,1) (0,1) (1,1) (1,2) (1,2) (2,2) (2,3) (3,3) (3,4) (4,4) (5,6)
    + [_case(FV_40_SPEC, 40, 128, 8, Tq, Tk) for Tq, Tk in ((130, 1), (256, 63), (130, 64), (256, 65), (130, 127), (256, 128), (130, 129), (256, 192), (130, 193),
                                                            (130, 256), (256, 321))]
    + [_case(FV_40_SPEC, 40, 205, 5, 130, 193)]                    # head = bid % 5; 205 * 5 = 1025 blocks
    # d = 80
    + [_case(FV_80, 80, 2, 8, Tq, Tk) for Tq, Tk in ((1, 1), (129, 64), (260, 65), (260, 154))] + [_case(FV_80, 80, 4, 8, 129, 77, kv_div=2)]
    # d = 160: in-lane row sum, 3-slot ring with counted vmcnt; 1, 2, 3 and 4 tiles
    + [_case(FV_160, 160, 2, 8, Tq, Tk) for Tq, Tk in ((129, 1), (1, 63), (260, 64), (129, 65), (1, 128), (260, 129), (129, 193))]
    # d = 128, one head, one entry, ldq = 256
    + [_case(FV_128, 128, 1, 1, Tq, Tk) for Tq, Tk in ((1, 64), (129, 65), (300, 192))])
SPLIT_CASES = tuple(_case(SPLITKV, 128, 1, Hh, Tq, Tk, nsplit=ns)
                    for ns, Tk, Hh in ((2, 128, 1), (3, 192, 2), (16, 1024, 1), (2, 384, 1)) for Tq in (1, 129))
# the shape of test_gated_exact_pass_small (also a row of CASES)
GATED = _case(FV_40_SPEC, 40, 128, 8, 130, 256)


def case_id(c):
    s = f"{FV_NAMES[c.variant].replace(' ', '_') if c.variant < 6 else 'splitkv'}-B{c.B}H{c.H}-Tq{c.Tq}-Tk{c.Tk}"
    return s + (f"-kvdiv{c.kv_div}" if c.kv_div > 1 else "") + (f"-ns{c.nsplit}" if c.nsplit > 1 else "")


def tiles(Tk):
    """-> (nfull, nt): 64-key tiles without padded keys / tiles."""
    return Tk // KV_TILE, -(-Tk // KV_TILE)


def expected_variant(c, flash40=0):
    """The rule of choose() in csrc/attn.hip, restated: what the table says each row reaches."""
    if c.d != 40:
        return {80: FV_80, 128: FV_128, 160: FV_160}[c.d]
    qb2 = c.B * c.H * (-(-c.Tq // 256)) >= 1024
    return FV_40_QB1 if not qb2 or flash40 == 1 else FV_40_SPEC if flash40 == 0 else FV_40_QB2


def kv_map(c):
    return torch.arange(c.B) // c.kv_div


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=256)          # the kinds of one case share its draws (callers copy: inputs() stacks)
def sample_x(c, b):
    """Sample b of a case: [max(Tq, Tk), 3C] f16, columns [q | k | v] (K / V entry e takes the k and v columns of sample e)."""
    return torch.randn(max(c.Tq, c.Tk), 3 * c.H * c.d, generator=rng(c.seed * 4096 + b)).to(H)


def spike_samples(c):
    """The samples that carry a spiked (row, key) pair; distinct K / V entries."""
    if c.B <= 2:
        return tuple(range(c.B))
    if c.B <= 4:
        return (0, c.B - 1)
    return (0, c.B // 2 + 13, c.B - 1)


def subset(c):
    """The samples the float64 reference is evaluated on: all of them up to 4, else the first, the last and every spiked one (also the gated test's)."""
    if c.B <= 4:
        return tuple(range(c.B))
    return tuple(sorted({0, c.B - 1, *spike_samples(c), *(s[0] for s in overflow_spikes(c))}))


def spikes(c, kind):
    """[(sample, query row, key)] of the spiked kinds: k[kv_map[sample], key] = SPIKE_GAIN * q[sample, row]."""
    if kind not in SPIKED:
        return []
    key = c.Tk - 1 if kind == "last_key" else KV_TILE * (tiles(c.Tk)[1] - 1)
    return [(b, (c.Tq - 1, c.Tq // 2, 0)[i % 3], key) for i, b in enumerate(spike_samples(c))]


OVERFLOW_GAIN, GUARD_GAIN, OVERFLOW_NORM2 = 3.2, 1.6, 44.0


def overflow_spikes(c):
    """[(sample, query row, key, head)] of the `overflow` kind (the shape GATED): within ONE head, the key is gain x q, the row of q scaled to
    |q_h|^2 = 44, so the score is 32 bits (gain 3.2) or 16 bits (gain 1.6) where the rest of the row stays below 7.  Key 73 is in tile 1 (the second of
    the first pair, right behind rebase(0, true)), key 232 in tile 3 (the second of the second pair).  The blocks of a launch are sample * H + head (one
    256-query block per sample and head): the first two spikes are blocks 42 and 43 -- one block of the 512-block gated pass (per = 2) redoes both, back to
    back on one LDS ring -- the third is the last block of the launch."""
    if (c.B, c.H, c.Tq, c.Tk) != (128, 8, 130, 256):
        return []
    return [(5, 7, 73, 2), (5, 129, 232, 3), (127, 64, 73, 7)]


def _anti_offset(c):
    return torch.randn(c.H * c.d, generator=rng(c.seed + 77)).to(H)


def inputs(c, kind, samples=None, gain=None):
    """-> q [n, Tq, C], k [ne, Tk, C], v [ne, Tk, C] f16 and emap: for the samples asked for (default: all B), the K / V entries they use (in order of first
    use) and emap[i] = index into k / v of samples[i]."""
    samples = tuple(range(c.B)) if samples is None else tuple(samples)
    C, km = c.H * c.d, kv_map(c).tolist()
    ents = sorted({km[b] for b in samples})
    xs = {b: sample_x(c, b) for b in set(samples) | set(ents)}
    q = torch.stack([xs[b][:c.Tq, :C] for b in samples]).clone()
    k = torch.stack([xs[e][:c.Tk, C:2 * C] for e in ents]).clone()
    v = torch.stack([xs[e][:c.Tk, 2 * C:] for e in ents]).clone()
    if kind == "peaked":
        q = (q.float() * PEAK_GAIN).to(H)
    elif kind in SPIKED:
        for b, row, key in spikes(c, kind):
            if b in samples:
                k[ents.index(km[b]), key] = (q[samples.index(b), row].float() * SPIKE_GAIN).to(H)
    elif kind == "v_ones":
        u = _anti_offset(c)
        v = torch.ones_like(v)
        k = (k.float() + u.float()).to(H)
        q[:, 0] = (u.float() * ANTI_GAIN).to(H)
        q[:, c.Tq - 1] = (u.float() * ANTI_GAIN).to(H)
    elif kind == "overflow":
        d = c.d
        for b, row, key, h in overflow_spikes(c):
            if b in samples:
                i, sl = samples.index(b), slice(h * d, (h + 1) * d)
                qh = q[i, row, sl].float()
                q[i, row, sl] = (qh * (OVERFLOW_NORM2 / qh.pow(2).sum()).sqrt()).to(H)
                k[ents.index(km[b]), key, sl] = (q[i, row, sl].float() * (OVERFLOW_GAIN if gain is None else gain)).to(H)
    elif kind != "noise":
        raise ValueError(kind)
    return q, k, v, torch.tensor([ents.index(km[b]) for b in samples])


def heads(t, c):
    return t.view(t.shape[0], t.shape[1], c.H, c.d)


# ------------------------------------------------------------------------------------------------------------------ reference and emulation
def f32_scale(d):
    """The `float` the callers pass: d ** -0.5 rounded to float32."""
    return torch.tensor(d ** -0.5, dtype=F32).item()


def scaled_q(q, scale):
    """The Q panel's values: f16(f32(q) * (f32(scale) * f32(log2 e))), the product of the two scalars taken in float32 (AttnPanels::qscale)."""
    qs = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    return (q.float() * qs).to(H)


def attention_ref(q, k, v, scale, kv_map, dt):
    """q [B,Tq,H,d], k / v [Bkv,Tk,H,d] f16 -> (out, A) [B,Tq,H,d] in dt: softmax(Qs K^T) V in base 2 and A = softmax(Qs K^T) |V|."""
    qs, kk, vv = scaled_q(q, scale).to(dt), k[kv_map].to(dt), v[kv_map].to(dt)
    s = torch.einsum("bqhd,bkhd->bhqk", qs, kk)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    return torch.einsum("bhqk,bkhd->bqhd", p, vv), torch.einsum("bhqk,bkhd->bqhd", p, vv.abs())


MUTATIONS = ("drop_last_key", "pad_key_counted", "last_row_from_its_neighbour", "v_keys_swapped")


def _swapped_keys(Tk):
    """Keys 4..7 and 8..11 of every group of 16 exchanged (where both exist): the in-tile key permutation of the V^T panel."""
    idx = torch.arange(Tk)
    for j in range(Tk):
        if j % 16 in (4, 5, 6, 7) and j + 4 < Tk:
            idx[j], idx[j + 4] = j + 4, j
    return idx


def mutation_applies(c, mutation):
    """A mutation that is the identity on a case proves nothing there: the last row needs a neighbour, the swap a key 8."""
    return c.Tk > 1 and (mutation != "last_row_from_its_neighbour" or c.Tq > 1) and (mutation != "v_keys_swapped" or c.Tk > 8)


def flash_emulated(q, k, v, scale, kv_map, off, nsplit=1, mutation=None):
    """The kernels' arithmetic (module docstring) -> out [B,Tq,H,d] f16.  mutation: one of MUTATIONS -- a defect the bound has to see."""
    qs, kk, vv = scaled_q(q, scale).float(), k[kv_map].float(), v[kv_map].float()
    Tq, Tk = q.shape[1], k.shape[1]
    if mutation == "v_keys_swapped":
        vv = vv[:, _swapped_keys(Tk)]
    chunk = Tk // nsplit
    parts, lses = [], []
    for ci in range(nsplit):
        ks, last = slice(ci * chunk, (ci + 1) * chunk), ci == nsplit - 1
        s = torch.einsum("bqhd,bkhd->bhqk", qs, kk[:, ks])
        m = (s.amax(-1, keepdim=True) + off).to(H).float()
        p = torch.exp2(s - m).to(H).float()
        if mutation == "drop_last_key" and last:
            p[..., -1] = 0
        den = p.sum(-1, keepdim=True)
        if mutation == "pad_key_counted" and last:
            den = den + torch.exp2(-m).to(H).float()          # a padded key: K = 0 -> score 0; V = 0 -> nothing in the numerator
        num = torch.einsum("bhqk,bkhd->bqhd", p, vv[:, ks])
        parts.append((num / den.permute(0, 2, 1, 3)).to(H))
        lses.append((m + torch.log2(den)).permute(0, 2, 1, 3))
    if nsplit == 1:
        out = parts[0]
    else:
        lse = torch.stack(lses)                                    # [S,B,Tq,H,1]
        w = torch.exp2(lse - lse.amax(0, keepdim=True))
        out = ((w * torch.stack(parts).float()).sum(0) / w.sum(0)).to(H)
    if mutation == "last_row_from_its_neighbour":
        out[:, Tq - 1] = out[:, Tq - 2]
    return out


def bound(ref, A, Tk, vmax, atol, split=False):
    cA = REL_ELEM + (2.0 ** -11 if split else 0.0)
    return REL_ELEM * ref.abs() + cA * A + Tk * 2.0 ** -22 * vmax + atol


def figures(got, ref, bnd):
    """-> (worst elementwise fraction |got - ref| / bound, worst-row rel-L2 over the d elements of one (sample, query, head), rel-L2).  A NaN or an inf in
    `got` gives an infinite fraction."""
    got = got.to(F64)
    diff = (got - ref).abs()
    frac = torch.where(diff == 0, torch.zeros_like(diff), diff / bnd)
    frac = torch.where(torch.isfinite(got), frac, torch.full_like(frac, float("inf")))
    row = (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-12)
    return frac.max().item(), torch.nan_to_num(row, nan=float("inf")).max().item(), rel_l2(got, ref)


Ref = namedtuple("Ref", "samples q k v emap ref A atol rms vmax bound")


@functools.lru_cache(maxsize=8)
def reference(c, kind, gain=None):
    """The float64 reference of a case and input kind on subset(c), its floor and its bound (cached: leave unchanged)."""
    samples = subset(c)
    q, k, v, emap = inputs(c, kind, samples, gain)
    q4, k4, v4, scale = heads(q, c), heads(k, c), heads(v, c), f32_scale(c.d)
    r64, A = attention_ref(q4, k4, v4, scale, emap, F64)
    r32, _ = attention_ref(q4, k4, v4, scale, emap, F32)
    atol = 4.0 * (r32.to(F64) - r64).abs().max().item() + SUB16
    vmax = v.float().abs().max().item()
    return Ref(samples, q4, k4, v4, emap, r64, A, atol, r64.pow(2).mean().sqrt().item(), vmax, bound(r64, A, c.Tk, vmax, atol, c.nsplit > 1))
