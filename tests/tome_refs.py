"""References of the leaf parity tests of the VidToMe match, normalise and row-mover kernels (tests/test_gpu_tome_leaves.py; pinned on the CPU by
tests/test_tome_refs_cpu.py).  torch / numpy on the CPU only, and every comparison the GPU file makes with them is a bit compare.

match      `exact_metric` draws tokens from {-1/8, 0, +1/8}: every dot product of two rows is a multiple of 2^-6 of magnitude <= C / 64 <= 20, exact in f32
           under any summation order and exactly representable in f16 (spacing 2^-6 in [16, 32)).  The kernel's f16 scores are therefore DEFINED, the data
           is full of exact ties, and the maps must equal `match_ref` -- the tie rule of include/tclight_hip.h written out -- with no excluded rows.
normalise  `normalize_ref` is oracle.vidtome._normalize(emulate_f16=True) with the norm taken in float64.  The kernel sums squares in f32: each lane adds
           its 8 NK products in sequence (NK = ceil(C / 512) chunk slots; the products of two f16 are exact, the first add is exact), a 6-level tree adds
           the 64 lanes.  That is at most 8 NK + 5 roundings of relative size 2^-24 on partial sums no larger than the (all-positive) total, so the f32 sum
           is within (8 NK + 5) 2^-24 of the true one, its root within half of that, and the f32 square root adds one rounding of 2^-25:
               margin(C) = (8 ceil(C / 512) + 6) 2^-25   (relative, on the norm).
           Only a row whose float64 norm lies within margin(C) of the midpoint of two neighbouring f16 values can round to the other neighbour; such a row
           is `ambiguous`, and must then equal the second candidate -- the quotient by that other neighbour -- as a whole.
movers     torch indexing.
"""
import math

import numpy as np
import torch

H, F32, F64, I32 = torch.float16, torch.float32, torch.float64, torch.int32
SENT16 = 0x7DEF         # f16 sentinel bit pattern (a NaN; tests/leaf_refs.py)


def rng(seed):
    return torch.Generator().manual_seed(seed)


def sentinel16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16).view(H)


def is_sentinel16(t):
    return bool((t.contiguous().view(torch.int16) == SENT16).all())


def f16_of_f64(t):
    """float64 -> f16 in ONE rounding (numpy converts directly; torch goes through float32)."""
    return torch.from_numpy(t.contiguous().numpy().astype(np.float16))


# ------------------------------------------------------------------------------------------------------------------ matching
def exact_metric(Bt, T, C, density, seed, dup=()):
    """f16 [Bt, T, C] with entries in {-1/8, 0, +1/8}, nonzero with probability `density`.  dup: ((b_to, t_to), (b_from, t_from)) pairs, applied in
    order: row (b_to, t_to) becomes a copy of row (b_from, t_from)."""
    g = rng(seed)
    sign = torch.randint(0, 2, (Bt, T, C), generator=g) * 2 - 1
    keep = torch.rand(Bt, T, C, generator=g) < density
    m = (sign * keep).to(H) / 8
    for (bt, tt), (bf, tf) in dup:
        m[bt, tt] = m[bf, tf]
    return m


def scores_f16(metric, a_pos, b_pos):
    """f16 scores [na, Bt * nb] of the f16 metric [Bt, T, C]: float64 products, one rounding, batch entries concatenated along dst at b * nb + j.
    Also returns whether every score survived the rounding unchanged."""
    m = metric.to(F64)
    s = m[:, a_pos.long()] @ m[:, b_pos.long()].transpose(1, 2)
    s16 = f16_of_f64(s)
    exact = bool((s16.to(F64) == s).all())
    return s16.permute(1, 0, 2).reshape(len(a_pos), -1), exact


def row_max_first(s):
    """[na, K] -> (row maximum, lowest column attaining it)."""
    s = s.to(F32)
    mx = s.max(dim=1).values
    col = torch.arange(s.shape[1])
    idx = torch.where(s == mx[:, None], col, s.shape[1]).min(dim=1).values
    return mx, idx


def row_max_slabs(metric, a_pos, b_pos, device="cpu", slab=1024):
    """The same for a case whose score matrix does not fit: float64 scores in slabs of src rows on `device` (exact-score inputs only: integer multiples
    of 2^-6, exact in any order).  -> (row maximum, lowest concatenated dst index attaining it, every score f16-exact, rows with a tied maximum), on the CPU."""
    m = metric.to(device).to(F64)
    a, b = a_pos.to(device).long(), b_pos.to(device).long()
    Bt, nb = m.shape[0], len(b)
    dst = m[:, b].transpose(1, 2)                                            # [Bt, C, nb]
    col = torch.arange(Bt * nb, device=device)
    mx, idx, exact, ties = [], [], True, 0
    for lo in range(0, len(a), slab):
        s = (m[:, a[lo:lo + slab]] @ dst).permute(1, 0, 2).reshape(-1, Bt * nb)
        exact = exact and bool((s.to(H).to(F64) == s).all())
        v = s.max(dim=1).values
        hit = s == v[:, None]
        mx.append(v.float().cpu())
        idx.append(torch.where(hit, col, Bt * nb).min(dim=1).values.cpu())
        ties += int((hit.sum(1) > 1).sum())
    return torch.cat(mx), torch.cat(idx), exact, ties


def maps_from_row_max(node_max, node_idx, a_pos, b_pos, r, T):
    """The map half of match_ref: from each src row's maximum and partner (lowest concatenated dst index attaining it) to (mrg, unm)."""
    na, nb, nun = len(a_pos), len(b_pos), len(a_pos) - r
    a_pos, b_pos = a_pos.long(), b_pos.long()
    # the r largest maxima, ties to the lowest src INDEX i: a stable descending sort over i = 0 .. na-1
    order = torch.from_numpy(np.argsort(-node_max.to(F64).numpy(), kind="stable"))
    merged = torch.zeros(na, dtype=torch.bool)
    merged[order[:r]] = True
    mrg = torch.full((nun + nb,), -1, dtype=torch.int64)
    unm = torch.full((T,), -1, dtype=torch.int64)
    unm[a_pos[merged]] = nun + node_idx[merged] % nb
    keep = a_pos[~merged]                                   # ascending i
    mrg[:nun] = keep
    unm[keep] = torch.arange(nun)
    mrg[nun:] = b_pos
    unm[b_pos] = nun + torch.arange(nb)
    return mrg.to(I32), unm.to(I32)


def match_ref(metric, a_pos, b_pos, r, T):
    """(mrg int32 [na - r + nb], unm int32 [T]) of tcl_tome_match_f16 (include/tclight_hip.h); unm is -1 where neither list names the position."""
    s, _ = scores_f16(metric, a_pos, b_pos)
    return maps_from_row_max(*row_max_first(s), a_pos, b_pos, r, T)


def tie_counts(s, r):
    """scores [na, K] -> (src rows whose maximum is attained by more than one concatenated dst index, rows holding the threshold score if that group
    straddles the cut at r, distinct maxima)."""
    s = s.to(F32)
    mx = s.max(dim=1).values
    match_ties, na = int(((s == mx[:, None]).sum(1) > 1).sum()), len(mx)
    cut = 0
    if 0 < r < na:
        thr = torch.sort(mx, descending=True).values[r - 1]
        above, group = int((mx > thr).sum()), int((mx == thr).sum())
        cut = group if above + group > r else 0
    return match_ties, cut, int(mx.unique().numel())


def r_values(na, node_max=None):
    """0, 1, na // 2, na - 1, na where na allows; with the reference's row maxima also one r that is certain to cut through a group of equal maxima
    (the median row's group if it has two rows, else the largest group): one row of that group merged, the others not."""
    rs = {0, 1, na // 2, na - 1, na} & set(range(na + 1))
    if node_max is not None and na >= 2:
        vals, counts = node_max.unique(return_counts=True)
        med = torch.sort(node_max, descending=True).values[na // 2]
        v = med if int(counts[vals == med]) >= 2 else vals[counts.argmax()]
        if int(counts[vals == v]) >= 2:
            rs.add(int((node_max > v).sum()) + 1)
    return sorted(rs)


# position layouts: -> (a_pos, b_pos, T[, affine hint])
def layout(kind, na, nb, seed=0):
    """Generic-entry layouts.  arange: [src | dst]; interleaved: src and dst mixed through a sequence 17 positions longer than na + nb (some positions
    belong to neither list); shuffled: a_pos of `arange` permuted (index order != position order); mixed: interleaved with both lists permuted."""
    g = rng(1000 + seed + na * 7 + nb)
    if kind in ("arange", "shuffled"):
        a, b, T = torch.arange(na), torch.arange(na, na + nb), na + nb
        if kind == "shuffled":
            a = a[torch.randperm(na, generator=g)]
    else:
        T = na + nb + 17
        used = torch.randperm(T, generator=g)[:na + nb].sort().values
        is_src = torch.zeros(na + nb, dtype=torch.bool)
        is_src[torch.randperm(na + nb, generator=g)[:na]] = True
        a, b = used[is_src], used[~is_src]
        if kind == "mixed":
            a, b = a[torch.randperm(na, generator=g)], b[torch.randperm(nb, generator=g)]
    return a.to(I32), b.to(I32), T


LAYOUTS = ("arange", "interleaved", "shuffled", "mixed")


def affine_layout(kind, na, nb):
    """Affine layouts, a_pos[i] = i < a_split ? i : i + a_gap, b_pos[j] = b0 + j: -> (a_pos, b_pos, T, (a_split, a_gap, b0))."""
    a_split, a_gap, b0 = {"first": (0, nb, 0), "middle": (na // 2, nb, na // 2), "last": (na, nb, na), "two_set": (na, 0, na)}[kind]
    i = torch.arange(na)
    a = torch.where(i < a_split, i, i + a_gap)
    return a.to(I32), (b0 + torch.arange(nb)).to(I32), na + nb, (a_split, a_gap, b0)


AFFINE_LAYOUTS = ("first", "middle", "last", "two_set")


def forced_ties(a_pos, b_pos, Bt):
    """`dup` list for exact_metric: (1) dst rows either side of the 32-, 64- and 128-row boundaries of the dst sweep are made equal and a src row is
    made equal to them (a row's score with itself is its maximum: no other row can match more of its nonzero entries), so that src row's maximum is
    attained on both sides of the boundary; (2) a src row meets its own copy at dst j0 of batch entry 0 and at a LOWER dst j1 of batch entry 1: the
    concatenated index of batch 0 is lower, batch 0 must win."""
    na, nb, dup, i = len(a_pos), len(b_pos), [], 0
    a, b = a_pos.tolist(), b_pos.tolist()
    for k in (32, 64, 128):
        if nb > k and i < na:
            for bt in range(Bt):                            # the same vector in every batch entry: each entry's scores tie at k - 1 and k
                dup.append(((bt, b[k - 1]), (0, b[k - 1])))
                dup.append(((bt, b[k]), (0, b[k - 1])))
                dup.append(((bt, a[i]), (0, b[k - 1])))
            i += 1
    if Bt >= 2 and nb >= 12 and i < na:
        j0, j1 = 9, 5
        dup.append(((1, b[j1]), (0, b[j0])))
        dup.append(((0, a[i]), (0, b[j0])))
        dup.append(((1, a[i]), (0, b[j0])))
    return dup


# (C, na, nb, Bt, density) of the generic-entry cases of the GPU file, table rows 1 and 2, and of the affine-entry cases
MATCH_CASES = ([(C, 300, 200, Bt, 1.0 if C == 320 and Bt == 2 else 0.25 if C != 1280 else 0.1) for C in (64, 320, 640, 1280) for Bt in (1, 2, 3)]
               + [(320, na, nb, 2, 0.25) for na, nb in ((1, 1), (1, 128), (31, 63), (31, 333), (128, 1), (128, 127), (128, 128), (129, 129),
                                                         (129, 1), (257, 63), (257, 129), (257, 333))])
AFFINE_CASES = ([(C, 300, 200, Bt, 0.25) for C in (320, 640) for Bt in (1, 2, 3)]
                + [(320, na, nb, 2, 0.25) for na, nb in ((1, 1), (1, 128), (31, 63), (31, 333), (128, 1), (128, 127), (128, 128), (129, 129), (129, 1),
                                                          (257, 63), (257, 129), (257, 333))]
                + [(320, 700, 1000, 2, 0.25), (640, 700, 1000, 2, 0.25)])
BIG_CASE = (64, 7168, 7168, 2, 0.5)     # ceil(na/128) ceil(nb/128) Bt / 3072 = 2.04: the generic kernel walks two src tiles per block


def match_case(C, na, nb, Bt, density, kind, affine=False):
    """-> dict(metric, a_pos, b_pos, T, aff) of one case and layout; the seed depends on the case alone."""
    if affine:
        a_pos, b_pos, T, aff = affine_layout(kind, na, nb)
    else:
        (a_pos, b_pos, T), aff = layout(kind, na, nb), None
    metric = exact_metric(Bt, T, C, density, C + 3 * na + 5 * nb + Bt, forced_ties(a_pos, b_pos, Bt))
    return dict(metric=metric, a_pos=a_pos, b_pos=b_pos, T=T, aff=aff)


# ------------------------------------------------------------------------------------------------------------------ normalise
NORM_C = (8, 64, 320, 520, 640, 1032, 1280, 1544, 2048)
NORM_ROWS = (1, 5, 16, 17, 67)
AMBIGUOUS_CAP = 0.05


def margin(C):
    return (8 * math.ceil(C / 512) + 6) * 2.0 ** -25


def normalize_input(rows, C):
    """N(0, s) rows with s from 2^-6 to 2^4 (log-uniform over the rows); rows >= 5: row 1 is one-hot (norm 3) and row 3 holds four 0.5 (norm 1)."""
    g = rng(C * 131 + rows)
    s = 2.0 ** (torch.rand(rows, 1, generator=g) * 10 - 6)
    s[0], s[-1] = 2.0 ** -6, 2.0 ** 4
    x = (torch.randn(rows, C, generator=g) * s).to(H)
    if rows >= 5:
        x[1] = 0
        x[1, C // 2] = 3.0
        x[3] = 0
        x[3, torch.tensor([0, 1, C // 2, C - 1])] = 0.5
    return x


def normalize_ref(x):
    """x f16 [rows, C] -> (expected f16, ambiguous bool [rows], alternative f16).  expected = (x / f16(|x|)) rounded to f16, the norm from float64;
    alternative divides by the f16 neighbour on the other side of the rounding midpoint nearest to the norm (meaningful on ambiguous rows only)."""
    C = x.shape[-1]
    n64 = x.to(F64).pow(2).sum(-1).sqrt()
    n16 = f16_of_f64(n64)
    n16np = n16.numpy()
    lo = torch.from_numpy(np.nextafter(n16np, np.float16(-np.inf))).to(F64)
    hi = torch.from_numpy(np.nextafter(n16np, np.float16(np.inf))).to(F64)
    mid_lo, mid_hi = (lo + n16.to(F64)) / 2, (hi + n16.to(F64)) / 2
    near_lo, near_hi = (n64 - mid_lo).abs() <= margin(C) * n64, (n64 - mid_hi).abs() <= margin(C) * n64
    ambiguous = (near_lo | near_hi) & (n64 > 0)
    other = torch.where(near_lo, lo, hi).to(H)
    expected = (x.float() / n16.float()[:, None]).to(H)
    alternative = (x.float() / other.float()[:, None]).to(H)
    return expected, ambiguous, alternative


def normalize_matches(got, expected, ambiguous, alternative):
    """Row-wise verdict: bit-equal to `expected`, or -- ambiguous rows only -- bit-equal to `alternative` as a whole row."""
    bits = lambda t: t.contiguous().view(torch.int16)
    ok = (bits(got) == bits(expected)).all(-1)
    alt = (bits(got) == bits(alternative)).all(-1)
    return ok | (ambiguous & alt)


# ------------------------------------------------------------------------------------------------------------------ row movers
def gather_rows_ref(s1, s2, map_):
    """out[b][p] = map[p] >= 0 ? s1[b][map[p]] : s2[b][~map[p]]; map None = copy of the first n rows (the caller slices)."""
    if map_ is None:
        return s1.clone()
    m = map_.long()
    out = s1[:, m.clamp_min(0)].clone()
    neg = m < 0
    if neg.any():
        out[:, neg] = s2[:, ~m[neg]]
    return out


def gather_add_ref(h, y, map_):
    """h[b][i] + y[b][map[i]]: one f32 add of two f16, one rounding."""
    return (h.float() + y[:, map_.long()].float()).to(H)


def index_compose_ref(outer, inner, off, n):
    idx = torch.arange(n) if inner is None else inner[:n].long()
    return outer[off + idx]
