"""CPU: the float64 reference of tests/attn_refs.py against torch's scaled_dot_product_attention, the case table against the kernels and tile counts it is
meant to reach, and the elementwise bound of the GPU leaf tests of csrc/attn.hip pinned from both sides: the emulated kernel arithmetic stays inside it on
every case and input kind, and four defects of the kind a flash kernel can have -- a dropped last key, a padded key in the row sum, a row stored from its
neighbour, two key blocks of V exchanged -- leave it on every case where they change anything.  A bound that a wrong kernel could meet then cannot pass
quietly."""
import pytest
import torch
import torch.nn.functional as F

import attn_refs as R

F64, F32, H = torch.float64, torch.float32, torch.float16
ALL = R.CASES + R.SPLIT_CASES
# the input kind each defect has to show on (all of these, on every case where the mutation applies): the spiked row's output IS the last key's value; V = 1
# with every valid key far below a padded key's score of 0; rows that differ; values that differ
CAUGHT_ON = {"drop_last_key": ("last_key",), "pad_key_counted": ("v_ones",), "last_row_from_its_neighbour": ("noise", "peaked"),
             "v_keys_swapped": ("noise", "peaked")}


def kinds_of(c):
    return R.SPLIT_KINDS if c.nsplit > 1 else R.KINDS


def test_reference_vs_torch_sdpa():
    for c in (R.CASES[9], R.CASES[26], R.SPLIT_CASES[3]):
        r = R.reference(c, "noise")
        qq, kk, vv = (t.to(F64).transpose(1, 2) for t in (r.q, r.k[r.emap], r.v[r.emap]))
        want = F.scaled_dot_product_attention(qq, kk, vv, scale=R.f32_scale(c.d)).transpose(1, 2)
        # the reference scales by the ROUNDED Q panel (f16(q * scale * log2 e)): a relative 2^-11 per q element, far above 1e-9
        assert (r.ref - want).abs().max().item() <= 2e-3 * want.abs().max().item()
        qs = R.scaled_q(r.q, R.f32_scale(c.d)).to(F64).transpose(1, 2)
        exact = F.scaled_dot_product_attention(qs, kk, vv, scale=0.6931471805599453).transpose(1, 2)       # ln 2: base 2 on the panel's own values
        assert (r.ref - exact).abs().max().item() <= 1e-9
        assert (r.A >= r.ref.abs() - 1e-12).all() and (r.A <= r.v.to(F64).abs().max() + 1e-12).all()


def test_table_reaches_what_it_names():
    ids = [R.case_id(c) for c in ALL]
    assert len(set(ids)) == len(ids)
    for c in R.CASES:
        assert R.expected_variant(c) == c.variant, c
    assert {c.variant for c in R.CASES} == {R.FV_40_SPEC, R.FV_40_QB1, R.FV_80, R.FV_128, R.FV_160}       # FV_40_QB2: the gated pass and TCL_FLASH40 = 5
    spec = [c for c in R.CASES if c.variant == R.FV_40_SPEC]
    assert all(R.expected_variant(c, 5) == R.FV_40_QB2 and R.expected_variant(c, 1) == R.FV_40_QB1 for c in spec)
    assert {R.tiles(c.Tk) for c in spec} >= {(0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (5, 6)}
    assert {c.Tk for c in spec} == {1, 63, 64, 65, 127, 128, 129, 192, 193, 256, 321} and {c.Tq for c in spec} == {130, 256} and any(c.H == 5 for c in spec)
    small = [c for c in R.CASES if c.variant == R.FV_40_QB1]
    assert sorted(c.Tk for c in small) == [1, 2, 63, 64, 65, 127, 128, 129, 192, 321]
    assert all(sum(c.Tq == t for c in small) >= 2 for t in (1, 127, 128, 129, 300))
    d80, d160, d128 = ([c for c in R.CASES if c.d == d] for d in (80, 160, 128))
    assert {c.Tq for c in d80} == {1, 129, 260} and {c.Tk for c in d80} == {1, 64, 65, 77, 154} and any(c.kv_div == 2 for c in d80)
    assert sorted(c.Tk for c in d160) == [1, 63, 64, 65, 128, 129, 193] and {R.tiles(c.Tk)[1] for c in d160} == {1, 2, 3, 4}
    assert {c.Tq for c in d128} == {1, 129, 300} and {c.Tk for c in d128} == {64, 65, 192} and all(c.layout == "ld256" and c.H == c.B == 1 for c in d128)
    assert {(c.nsplit, c.Tk) for c in R.SPLIT_CASES} == {(2, 128), (3, 192), (16, 1024), (2, 384)} and {c.Tq for c in R.SPLIT_CASES} == {1, 129}
    assert all(c.Tk % (64 * c.nsplit) == 0 for c in R.SPLIT_CASES)
    assert R.GATED in R.CASES and max(c.B * c.H * c.Tq * c.Tk for c in R.CASES) == 128 * 8 * 256 * 321
    for c in ALL:                                                                  # the subset holds the first, the last and every spiked sample
        assert {0, c.B - 1, *R.spike_samples(c)} <= set(R.subset(c))
        km = R.kv_map(c).tolist()
        assert len({km[b] for b in R.spike_samples(c)}) == len(R.spike_samples(c))


def test_spiked_rows_take_the_spiked_key():
    """In the spiked kinds the chosen row's output is the spiked key's value to within 2 % of max|v|: the key really dominates, at the place the kind names."""
    for c in ALL:
        for kind in (("last_key",) if c.nsplit > 1 else R.SPIKED):
            r = R.reference(c, kind)
            nt = R.tiles(c.Tk)[1]
            for b, row, key in R.spikes(c, kind):
                assert key == (c.Tk - 1 if kind == "last_key" else 64 * (nt - 1)) and 0 <= row < c.Tq
                i = r.samples.index(b)
                assert (r.ref[i, row] - r.v[r.emap[i], key].to(F64)).abs().max().item() <= 0.02 * r.vmax, (R.case_id(c), kind, b, row)
            if c.nsplit > 1:
                assert all(key >= c.Tk - c.Tk // c.nsplit for _, _, key in R.spikes(c, kind))       # in the last chunk: one chunk dominates the merge


@pytest.mark.parametrize("c", ALL, ids=R.case_id)
def test_emulation_inside_the_bound_and_mutations_outside(c):
    worst = 0.0
    for kind in kinds_of(c):
        r = R.reference(c, kind)
        assert r.atol <= R.ATOL_CAP * r.rms, (kind, r.atol, r.rms)
        if kind == "v_ones":
            assert (r.ref - 1).abs().max().item() <= 1e-12
        for off in (0.0, 3.0):
            got = R.flash_emulated(r.q, r.k, r.v, R.f32_scale(c.d), r.emap, off, c.nsplit)
            frac, row, rel = R.figures(got, r.ref, r.bound)
            worst = max(worst, frac)
            assert frac <= 1.0, (kind, off, frac, row, rel)
        for mutation in R.MUTATIONS:
            if kind in CAUGHT_ON[mutation] and R.mutation_applies(c, mutation):
                for off in (0.0, 3.0):
                    bad = R.flash_emulated(r.q, r.k, r.v, R.f32_scale(c.d), r.emap, off, c.nsplit, mutation)
                    frac = R.figures(bad, r.ref, r.bound)[0]
                    assert frac > 1.0, (mutation, kind, off, frac)
    print(f"[attn bound] {R.case_id(c)}: emulation's worst elementwise fraction {worst:.3f}")


def test_every_mutation_is_tried_on_every_case_it_changes():
    for c in ALL:
        for mutation in R.MUTATIONS:
            if R.mutation_applies(c, mutation):
                assert set(CAUGHT_ON[mutation]) & set(kinds_of(c)), (R.case_id(c), mutation)
            else:
                assert c.Tk == 1 or (mutation == "last_row_from_its_neighbour" and c.Tq == 1) or (mutation == "v_keys_swapped" and c.Tk <= 8)
    idx = R._swapped_keys(21).tolist()
    assert idx[:16] == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15] and idx[16:] == [16, 17, 18, 19, 20]


def test_overflow_input_overflows_where_it_says():
    """The speculative kernel's shift sits at most 3 bits above, and less than 1 bit below, the largest score a row has seen before a pair of tiles (tile 0:
    its own maximum).  A score >= 19 bits above that maximum overflows f16 P for certain (the block must be flagged); one < 15 bits above cannot.  With gain
    3.2 the three spiked (row, key, head) triples are beyond 19 + 1 and every score of the sampled blocks without a spike is below 15 - 1; with gain 1.6 all
    scores are.  (Samples outside the subset hold noise alone: their scores rise a few bits.)"""
    c = R.GATED
    spikes = R.overflow_spikes(c)
    assert len(spikes) == 3 and R.tiles(c.Tk) == (4, 4)
    blocks = [b * c.H + h for b, _, _, h in spikes]
    assert blocks[0] // 2 == blocks[1] // 2 and blocks[0] != blocks[1] and blocks[2] == c.B * c.H - 1        # per = 2: one gated block redoes two items
    assert [k // 64 for _, _, k, _ in spikes] == [1, 3, 1]
    for gain, flagged in ((R.OVERFLOW_GAIN, True), (R.GUARD_GAIN, False)):
        r = R.reference(c, "overflow", gain)
        s = torch.einsum("bqhd,bkhd->bhqk", R.scaled_q(r.q, R.f32_scale(c.d)).to(F64), r.k[r.emap].to(F64))     # [n,H,Tq,Tk]
        before = torch.stack([s[..., :64].amax(-1), s[..., :128].amax(-1)], -1)                                    # the maximum a pair starts from
        rise = torch.cat([s[..., 64:128] - before[..., :1], s[..., 128:] - before[..., 1:]], -1)                  # keys 64 .. 255
        hit = torch.zeros_like(rise, dtype=torch.bool)
        for b, row, key, h in spikes:
            hit[r.samples.index(b), h, row, key - 64] = True
        print(f"[attn overflow] gain {gain}: spiked scores rise {[round(x, 1) for x in rise[hit].tolist()]} bits, all others at most {rise[~hit].max().item():.1f}")
        if flagged:                    # a flag is per block: inside a spiked (sample, head) anything may happen, every other block must stay clean
            assert rise[hit].min().item() >= 20.0, rise[hit]
            for b, _, _, h in spikes:
                rise[r.samples.index(b), h] = -1e9
        assert rise.max().item() <= 14.0
        got = R.flash_emulated(r.q, r.k, r.v, R.f32_scale(c.d), r.emap, 0.0)
        assert R.figures(got, r.ref, r.bound)[0] <= 1.0 and r.atol <= R.ATOL_CAP * r.rms
