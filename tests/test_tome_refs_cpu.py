"""CPU: pins the references of tests/test_gpu_tome_leaves.py (tests/tome_refs.py) -- match_ref states the rule oracle.vidtome._match_one states, every
matching case of the GPU file has exact scores and real ties, and the normalise inputs leave at most 5 % of their rows undecided."""
import pytest
import torch

import tome_refs as R
from oracle import vidtome as OV

F64, H = torch.float64, torch.float16


def _oracle_maps(s, a_pos, b_pos, r, T):
    mrg, unm = OV._match_one(s.float(), a_pos.long(), b_pos.long(), r, T)
    return mrg, unm


@pytest.mark.parametrize("kind", R.LAYOUTS + R.AFFINE_LAYOUTS)
@pytest.mark.parametrize("C,na,nb,Bt,density", [(64, 40, 30, 1, 0.5), (320, 70, 50, 2, 0.25), (320, 33, 130, 3, 1.0), (640, 5, 1, 2, 0.25), (64, 1, 7, 3, 0.5)])
def test_match_ref_states_the_oracle_rule(C, na, nb, Bt, density, kind):
    """Same token restored at every position, same dst half; the unmerged src slots are a permutation (the oracle orders them by score, the kernel
    and match_ref by src index)."""
    c = R.match_case(C, na, nb, Bt, density, kind, affine=kind in R.AFFINE_LAYOUTS)
    a_pos, b_pos, T = c["a_pos"], c["b_pos"], c["T"]
    s, exact = R.scores_f16(c["metric"], a_pos, b_pos)
    assert exact
    for r in R.r_values(na):
        mrg, unm = R.match_ref(c["metric"], a_pos, b_pos, r, T)
        omrg, ounm = _oracle_maps(s, a_pos, b_pos, r, T)
        nun = na - r
        mrg, unm = mrg.long(), unm.long()
        assert mrg.shape == omrg.shape == (nun + nb,) and unm.shape == ounm.shape == (T,)
        named = torch.zeros(T, dtype=torch.bool)
        named[a_pos.long()] = True
        named[b_pos.long()] = True
        assert torch.equal(unm < 0, ~named) and torch.equal(ounm < 0, ~named)
        assert torch.equal(mrg[unm[named]], omrg[ounm[named]]), (kind, r)                    # the position every token is restored from
        assert torch.equal(mrg[nun:], omrg[nun:]) and torch.equal(unm[b_pos.long()], ounm[b_pos.long()])
        assert torch.equal(mrg[:nun].sort().values, omrg[:nun].sort().values)
        # match_ref's own order: unmerged src in ascending index i, each in the slot it is read back from
        keep = torch.tensor([i for i in range(na) if unm[a_pos[i]] < nun], dtype=torch.long)
        assert torch.equal(mrg[:nun], a_pos.long()[keep]) and torch.equal(unm[a_pos.long()[keep]], torch.arange(nun))


def test_match_ref_tie_rule_by_hand():
    """Two dst rows per batch entry, all equal to the src rows: every score ties.  Partner = dst 0 (batch 0); the cut takes the lowest src INDEX, which
    with a_pos = [4, 2, 3] is position 4, not the lowest position."""
    metric = torch.zeros(2, 6, 64, dtype=H)
    metric[..., 0] = 0.125
    a_pos, b_pos = torch.tensor([4, 2, 3], dtype=torch.int32), torch.tensor([5, 0], dtype=torch.int32)
    mrg, unm = R.match_ref(metric, a_pos, b_pos, 1, 6)
    assert mrg.tolist() == [2, 3, 5, 0] and unm.tolist() == [3, -1, 0, 1, 2, 2]


def _cases():
    out = [(c, k, False) for c in R.MATCH_CASES for k in R.LAYOUTS] + [(c, k, True) for c in R.AFFINE_CASES for k in R.AFFINE_LAYOUTS]
    return out


def test_scores_are_exact_and_every_case_has_ties():
    """Every score of every case of the GPU file round-trips float64 -> f16 -> float64; every case has match ties (when it has two dst rows: with
    one, every partner is that row whichever batch entry wins) and at least one r whose cut falls inside a group of equal maxima (when it has two src rows).  `-s` prints the counts."""
    for (C, na, nb, Bt, density), kind, affine in _cases():
        c = R.match_case(C, na, nb, Bt, density, kind, affine)
        s, exact = R.scores_f16(c["metric"], c["a_pos"], c["b_pos"])
        assert exact, (C, na, nb, Bt, kind)
        counts = {r: R.tie_counts(s, r) for r in R.r_values(na, R.row_max_first(s)[0])}
        mt, cut, distinct = counts[na // 2][0], max(v[1] for v in counts.values()), counts[na // 2][2]
        print(f"[tome ties] C {C} na {na} nb {nb} Bt {Bt} density {density} {'affine ' if affine else ''}{kind}: {mt} of {na} rows with a tied maximum, "
              f"{counts[na // 2][1]} rows on the cut at r = na // 2 (most over the r used: {cut}), {distinct} distinct maxima")
        if nb >= 2:
            assert mt > 0, f"no match tie: C {C} na {na} nb {nb} Bt {Bt} {kind}: {mt} tied rows"
        if na >= 2:
            assert cut > 0, f"no cut tie: C {C} na {na} nb {nb} Bt {Bt} {kind}: {cut} rows on the threshold"


def test_big_case_scores_are_exact_and_tied():
    C, na, nb, Bt, density = R.BIG_CASE
    assert -(-na // 128) * -(-nb // 128) * Bt // 3072 >= 2 and (na - 128) // 128 * (-(-(nb - 128) // 128)) * Bt // 3072 < 2    # the smallest such size
    c = R.match_case(C, na, nb, Bt, density, "shuffled")
    mx, idx, exact, ties = R.row_max_slabs(c["metric"], c["a_pos"], c["b_pos"])
    assert exact
    thr = torch.sort(mx, descending=True).values[na // 2 - 1]
    cut = int((mx == thr).sum())
    print(f"[tome ties] big case C {C} na {na} nb {nb} Bt {Bt}: {ties} rows with a tied maximum, {cut} rows on the cut at r = na // 2, {mx.unique().numel()} distinct maxima")
    assert ties > 0 and cut > 1 and int((mx > thr).sum()) + cut > na // 2
    # the slab form and the one-piece form agree (on the first slab of src rows)
    s, _ = R.scores_f16(c["metric"], c["a_pos"][:256], c["b_pos"])
    m2, i2 = R.row_max_first(s)
    assert torch.equal(m2, mx[:256]) and torch.equal(i2, idx[:256])


def test_forced_ties_are_where_they_should_be():
    """The duplicated dst rows either side of the 32 / 64 / 128 boundaries and in two batch entries: the src row built for each has its maximum on both,
    and match_ref sends it to the lower concatenated index."""
    C, na, nb, Bt = 320, 300, 200, 2
    c = R.match_case(C, na, nb, Bt, 0.25, "mixed")
    s, _ = R.scores_f16(c["metric"], c["a_pos"], c["b_pos"])
    mx, idx = R.row_max_first(s)
    for i, k in enumerate((32, 64, 128)):
        assert s[i, k - 1] == mx[i] and s[i, k] == mx[i] and s[i, nb + k - 1] == mx[i] and idx[i] <= k - 1
    assert s[3, 9] == mx[3] and s[3, nb + 5] == mx[3] and idx[3] <= 9       # batch 0's dst 9 before batch 1's dst 5


# ------------------------------------------------------------------------------------------------------------------ normalise
def test_normalize_ref_is_the_oracle_and_mostly_decided():
    """expected = oracle.vidtome._normalize(emulate_f16=True), bit for bit, on every input of the GPU file; at most 5 % of the rows of each C are
    ambiguous.  Expected: a norm is ambiguous when it falls within margin(C) |x| of one of the midpoints, which lie one f16 ulp apart, and the relative
    ulp runs from 2^-10 to 2^-11 over a binade (2^-10.5 in the geometric mean): 2 margin / 2^-10.5 = 0.12 % (C <= 512) to 0.33 % (C > 1536).  Even at
    the finest ulp, 2 margin / 2^-11 is 0.17-0.46 %; a fraction of 1-2 % would need a margin several times wider than the derived one, and is no reason
    to widen it.  5 % is a cap on what the GPU test may leave undecided, not the expectation."""
    for C in R.NORM_C:
        amb = total = 0
        for rows in R.NORM_ROWS:
            x = R.normalize_input(rows, C)
            expected, ambiguous, alternative = R.normalize_ref(x)
            want = OV._normalize(x, True).to(H)
            assert torch.equal(expected.view(torch.int16), want.view(torch.int16)), (C, rows)
            assert not torch.isnan(expected.float()).any()
            amb, total = amb + int(ambiguous.sum()), total + rows
            if rows >= 5:                              # exactly known norms 3 and 1: never ambiguous, quotients exact
                assert not ambiguous[1] and not ambiguous[3]
                assert expected[1, C // 2] == 1.0 and expected[1].float().abs().sum() == 1.0
                assert torch.equal(expected[3], x[3])
            print(f"[tome normalise] C {C} rows {rows}: {int(ambiguous.sum())} ambiguous rows")
        print(f"[tome normalise] C {C}: {amb} of {total} rows ambiguous ({amb / total:.2%}); margin {R.margin(C):.3e}")
        assert amb <= R.AMBIGUOUS_CAP * total, (C, amb, total)


def test_normalize_ref_marks_a_midpoint_row():
    """A row built to have its norm within margin(C) of the midpoint of the f16 values 1 and 1 + 2^-10 (one entry 1, 63 entries near a with
    1 + 63 a^2 = midpoint^2, nudged by f16 ulps) is found ambiguous, its alternative divides by the other neighbour, and normalize_matches accepts
    those two rows and no mixture of them."""
    C = 64
    n_lo, n_hi = 1.0, 1.0 + 2.0 ** -10
    mid = (n_lo + n_hi) / 2
    a = ((mid * mid - 1.0) / 63) ** 0.5
    best = None
    for da in range(-40, 41):
        for k in range(0, 64):
            x = torch.zeros(1, C, dtype=H)
            x[0, 0] = 1.0
            x[0, 1:] = torch.tensor(a, dtype=H)
            bits = x.view(torch.int16)
            bits[0, 1:1 + k] += da
            n = x.to(F64).pow(2).sum().sqrt().item()
            if best is None or abs(n - mid) < abs(best[0] - mid):
                best = (n, x.clone())
    n, x = best
    assert abs(n - mid) <= R.margin(C) * n, (n, mid)
    expected, ambiguous, alternative = R.normalize_ref(x)
    assert bool(ambiguous[0])
    q_lo, q_hi = (x.float() / n_lo).to(H), (x.float() / torch.tensor(n_hi, dtype=H).float()).to(H)
    both = {tuple(expected.view(torch.int16)[0].tolist()), tuple(alternative.view(torch.int16)[0].tolist())}
    assert both == {tuple(q_lo.view(torch.int16)[0].tolist()), tuple(q_hi.view(torch.int16)[0].tolist())} and len(both) == 2
    assert R.normalize_matches(q_lo, expected, ambiguous, alternative).all() and R.normalize_matches(q_hi, expected, ambiguous, alternative).all()
    mixed = q_lo.clone()
    mixed[0, 1:] = q_hi[0, 1:]
    if not (torch.equal(mixed, q_lo) or torch.equal(mixed, q_hi)):
        assert not R.normalize_matches(mixed, expected, ambiguous, alternative).any()      # a row must follow ONE candidate
    undecided = torch.zeros(1, dtype=torch.bool)                                           # the same row, not marked: only `expected` passes
    assert int(R.normalize_matches(q_lo, expected, undecided, alternative).sum()) + int(R.normalize_matches(q_hi, expected, undecided, alternative).sum()) == 1


# ------------------------------------------------------------------------------------------------------------------ row movers
def test_mover_refs():
    s1 = torch.arange(2 * 4 * 8).reshape(2, 4, 8).to(H)
    s2 = -s1
    out = R.gather_rows_ref(s1, s2, torch.tensor([3, -1, 0, -4, 3]))
    assert torch.equal(out[:, 0], s1[:, 3]) and torch.equal(out[:, 1], s2[:, 0]) and torch.equal(out[:, 3], s2[:, 3]) and torch.equal(out[:, 4], s1[:, 3])
    assert torch.equal(R.gather_rows_ref(s1, None, None), s1)
    h = torch.tensor([[[2048.0, -0.0, 0.0, 1.0]]], dtype=H)
    y = torch.tensor([[[1.0, 0.0, -0.0, 2.0 ** -11]]], dtype=H)
    got = R.gather_add_ref(h, y, torch.tensor([0]))
    assert got[0, 0].tolist() == [2048.0, 0.0, 0.0, 1.0]          # 2049 rounds to even, 1 + 2^-11 rounds to even
    outer = torch.tensor([5, 6, 7, 8, 9])
    assert R.index_compose_ref(outer, torch.tensor([2, 0, 1]), 1, 3).tolist() == [8, 6, 7]
    assert R.index_compose_ref(outer, None, 2, 3).tolist() == [7, 8, 9]
