"""GPU: leaf parity of the VidToMe kernels of csrc/merge.hip -- match (both score kernels, threshold select, maps), normalise, the row movers and
index_compose -- each through the C ABI against tests/tome_refs.py (pinned by tests/test_tome_refs_cpu.py).

Every assertion is a bit compare.  Matching runs on tokens from {-1/8, 0, +1/8}: every score is exact in f32 in any order and representable in f16, a
third of the rows have a tied maximum and dozens sit on the cut, so the maps are DEFINED by the rule of include/tclight_hip.h -- highest score, lowest
concatenated dst index (batch entry 0 first), equal maxima cut in ascending src index, unmerged src in index order -- and must equal match_ref.  The one
place where two results pass is a normalise row whose float64 norm lies within margin(C) of an f16 rounding midpoint (tome_refs.normalize_ref): it may
follow either neighbouring norm, as a whole row; at most 5 % of the rows of a C may be such rows.
Outputs and padding are prefilled with a sentinel (f16 0x7DEF, int -1) and checked afterwards; `-s` prints the figures kept in
profiles/tome_leaf_parity.txt."""
import pytest
import torch

import tome_refs as R

pytestmark = pytest.mark.gpu
H, I32 = torch.float16, torch.int32
PAD = 8                                  # int32 sentinels behind mrg and unm


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(t):
    return t.contiguous().cuda()


def bits(t):
    return t.contiguous().view(torch.int16)


def eq16(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def new_ws(L, na):
    return torch.zeros(L.tcl_tome_match_workspace_bytes(na), dtype=torch.uint8, device="cuda")


def ws_clean(ws):
    """All-zero except ints 768..771 of the control block (tickets, zero again; thr; take) -- as test_tome_match_strip_kernel_equals_tile_kernel asserts it."""
    return not ws[:3072].any() and not ws[3072 + 16:].any()


class Case:
    """One matching case on the device with its reference row maxima (computed once, shared by every r and entry point)."""

    def __init__(self, C, na, nb, Bt, density, kind, affine=False, big=False):
        c = R.match_case(C, na, nb, Bt, density, kind, affine)
        self.C, self.na, self.nb, self.Bt, self.T, self.aff, self.kind = C, na, nb, Bt, c["T"], c["aff"], kind
        self.a_pos, self.b_pos = c["a_pos"], c["b_pos"]
        self.metric, self.a_dev, self.b_dev = dev(c["metric"]), dev(c["a_pos"]), dev(c["b_pos"])
        if big:
            self.mx, self.idx, exact, _ = R.row_max_slabs(self.metric, self.a_pos, self.b_pos, device="cuda")
            assert exact
        else:
            self.mx, self.idx = R.row_max_first(R.scores_f16(c["metric"], self.a_pos, self.b_pos)[0])
        self.rs = R.r_values(na, self.mx)

    def ref(self, r):
        return R.maps_from_row_max(self.mx, self.idx, self.a_pos, self.b_pos, r, self.T)

    def run(self, L, r, ws, affine):
        mrg = torch.full((self.na - r + self.nb + PAD,), -1, dtype=I32, device="cuda")
        unm = torch.full((self.T + PAD,), -1, dtype=I32, device="cuda")
        args = (self.metric, self.T * self.C, self.Bt, self.C, self.a_dev, self.na, self.b_dev, self.nb, r)
        if affine:
            L.tcl_tome_match_affine_f16(*args, *self.aff, mrg, unm, ws, st())
        else:
            L.tcl_tome_match_f16(*args, mrg, unm, ws, st())
        torch.cuda.synchronize()
        return mrg.cpu(), unm.cpu()

    def check(self, L, r, ws, affine, note=""):
        mrg, unm = self.run(L, r, ws, affine)
        want_mrg, want_unm = self.ref(r)
        what = (self.C, self.na, self.nb, self.Bt, self.kind, "affine" if affine else "generic", f"r={r}", note)
        assert torch.equal(unm[:-PAD], want_unm), ("unm", what, int((unm[:-PAD] != want_unm).sum()))
        assert torch.equal(mrg[:-PAD], want_mrg), ("mrg", what, int((mrg[:-PAD] != want_mrg).sum()))
        assert (mrg[-PAD:] == -1).all() and (unm[-PAD:] == -1).all(), ("written past the maps", what)
        assert ws_clean(ws), ("workspace not left clean", what)


# ================================================================================================================== matching
@pytest.mark.parametrize("C,na,nb,Bt,density", R.MATCH_CASES)
def test_match_generic(L, C, na, nb, Bt, density):
    """tcl_tome_match_f16 == match_ref for every r and four position layouts (arange; src / dst interleaved with positions in neither list, which keep
    their -1; a_pos shuffled; both shuffled).  One workspace, zeroed once, serves every call of the test."""
    ws = new_ws(L, na)
    for kind in R.LAYOUTS:
        c = Case(C, na, nb, Bt, density, kind)
        for r in c.rs:
            c.check(L, r, ws, affine=False)


@pytest.mark.parametrize("C,na,nb,Bt,density", R.AFFINE_CASES)
def test_match_affine(L, C, na, nb, Bt, density):
    """tcl_tome_match_affine_f16 == match_ref with the dst frame first, in the middle, last and in the two-set form, with the C = 640 strip kernel
    off and on; and the generic entry on the same arrays.  nb < 128 (nb = 1 and na = 1 among them) hands over to the tile kernel; 700 x 1000 splits
    the dst sweep and moves its last tile back."""
    ws = new_ws(L, na)
    try:
        for strip640 in (0, 1):
            L.tcl_tome_strip640(strip640)
            for kind in R.AFFINE_LAYOUTS:
                c = Case(C, na, nb, Bt, density, kind, affine=True)
                for r in c.rs:
                    c.check(L, r, ws, affine=True, note=f"strip640={strip640}")
                    if strip640 == 0:
                        c.check(L, r, ws, affine=False)
    finally:
        L.tcl_tome_strip640(0)


def test_match_more_than_one_src_tile_per_block(L):
    """C = 64, na = nb = 7168, Bt = 2: the smallest square case in which a block of the generic kernel walks two src tiles, its DMA ring running on
    across the tile boundary after an epilogue's atomics.  Reference row maxima in float64 on the GPU in slabs (integer multiples of 2^-6: exact in
    any order)."""
    C, na, nb, Bt, density = R.BIG_CASE
    assert -(-na // 128) * -(-nb // 128) * Bt // 3072 == 2
    ws = new_ws(L, na)
    for kind in R.LAYOUTS:
        c = Case(C, na, nb, Bt, density, kind, big=True)
        for r in c.rs:
            c.check(L, r, ws, affine=False)


def test_match_workspace_reused_across_sizes(L):
    """One workspace sized for na = 700, zeroed once: na = 700, then 257, then 700 again, both entries -- the maps do not change."""
    ws = new_ws(L, 700)
    big, small = Case(320, 700, 1000, 2, 0.25, "middle", affine=True), Case(320, 257, 129, 2, 0.25, "middle", affine=True)
    for affine in (False, True):
        first = big.run(L, 350, ws, affine)
        big.check(L, 350, ws, affine)
        small.check(L, 128, ws, affine)
        small.check(L, 257, ws, affine)
        big.check(L, 350, ws, affine)
        again = big.run(L, 350, ws, affine)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_match_refused_arguments(L):
    """TCL_EINVAL before any launch: maps and workspace untouched."""
    c = Case(320, 31, 63, 2, 0.25, "arange")
    ws = new_ws(L, 65536)
    mrg = torch.full((256,), -1, dtype=I32, device="cuda")
    unm = torch.full((256,), -1, dtype=I32, device="cuda")
    m, bs, a, b = c.metric, c.T * c.C, c.a_dev, c.b_dev
    bad = [
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 31, b, 63, 32, mrg, unm, ws, st()),            # r > na
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 31, b, 63, -1, mrg, unm, ws, st()),            # r < 0
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 0, b, 63, 0, mrg, unm, ws, st()),              # na = 0
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 31, b, 0, 1, mrg, unm, ws, st()),              # nb = 0
        lambda: L.tcl_tome_match_f16(m, bs, 2, 328, a, 31, b, 63, 1, mrg, unm, ws, st()),             # C % 64
        lambda: L.tcl_tome_match_f16(m, bs, 2, 32, a, 31, b, 63, 1, mrg, unm, ws, st()),
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 65537, b, 63, 1, mrg, unm, ws, st()),          # na > 65536
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 31, b, 63, 1, 0, unm, ws, st()),               # null maps
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 31, b, 63, 1, mrg, 0, ws, st()),
        lambda: L.tcl_tome_match_f16(m, bs, 0, 320, a, 31, b, 63, 1, mrg, unm, ws, st()),             # Bt = 0
        lambda: L.tcl_tome_match_f16(m, bs, 2, 320, a, 31, b, 63, 1, mrg, unm, 0, st()),              # no workspace
        lambda: L.tcl_tome_match_affine_f16(m, bs, 2, 320, a, 31, b, 63, 32, 31, 0, 31, mrg, unm, ws, st()),
        lambda: L.tcl_tome_match_affine_f16(m, bs, 2, 320, a, 31, b, 63, 1, -1, 0, 31, mrg, unm, ws, st()),
        lambda: L.tcl_tome_match_affine_f16(m, bs, 2, 320, a, 31, b, 63, 1, 31, -1, 31, mrg, unm, ws, st()),
        lambda: L.tcl_tome_match_affine_f16(m, bs, 2, 320, a, 31, b, 63, 1, 31, 0, -1, mrg, unm, ws, st()),
        lambda: L.tcl_tome_match_affine_f16(m, bs, 2, 320, a, 31, b, 63, 1, 31, 0, 31, 0, unm, ws, st()),
    ]
    for call in bad:
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            call()
    torch.cuda.synchronize()
    assert (mrg == -1).all() and (unm == -1).all() and not ws.any()


# ================================================================================================================== normalise
def _normalize(L, x, extra=3):
    rows, C = x.shape
    y = dev(R.sentinel16(rows + extra, C))
    L.tcl_tome_normalize_f16(dev(x), y, rows, C, st())
    torch.cuda.synchronize()
    y = y.cpu()
    assert R.is_sentinel16(y[rows:]), ("written past the last row", rows, C)
    return y[:rows]


@pytest.mark.parametrize("C", R.NORM_C)
def test_normalize(L, C):
    """Bit-equal to normalize_ref at 1, 5, 16, 17 and 67 rows (one wave partly filled, one block, one block and a row, five blocks); rows 1 and 3 have
    the exactly known norms 3 and 1 and are never ambiguous."""
    amb = total = alt_used = 0
    for rows in R.NORM_ROWS:
        x = R.normalize_input(rows, C)
        expected, ambiguous, alternative = R.normalize_ref(x)
        got = _normalize(L, x)
        ok = R.normalize_matches(got, expected, ambiguous, alternative)
        first = (bits(got) == bits(expected)).all(-1)
        amb, total, alt_used = amb + int(ambiguous.sum()), total + rows, alt_used + int((ok & ~first).sum())
        assert ok.all(), (C, rows, "rows that match neither candidate", torch.nonzero(~ok).flatten().tolist(), "ambiguous", torch.nonzero(ambiguous).flatten().tolist())
        if rows >= 5:
            assert not ambiguous[1] and not ambiguous[3] and first[1] and first[3]
    print(f"[tome normalise] C {C}: {amb} of {total} rows ambiguous ({amb / total:.2%}), {alt_used} of them followed the other neighbour; margin {R.margin(C):.3e}")
    assert amb <= R.AMBIGUOUS_CAP * total


@pytest.mark.parametrize("C", R.NORM_C)
def test_normalize_zero_row(L, C):
    """An all-zero row in the middle of a wave's four rows (row 6 of 17: the wave holds rows 4..7) is NaN, as the oracle's; every other row is unaffected."""
    x = R.normalize_input(17, C)
    x[6] = 0
    expected, ambiguous, alternative = R.normalize_ref(x)
    got = _normalize(L, x)
    assert torch.isnan(expected[6].float()).all() and torch.isnan(got[6].float()).all()
    others = torch.arange(17) != 6
    assert R.normalize_matches(got, expected, ambiguous, alternative)[others].all()
    assert not torch.isnan(got[others].float()).any()


def test_normalize_refused_arguments(L):
    x, y = dev(torch.ones(4, 2056, dtype=H)), dev(R.sentinel16(4, 2056))
    for rows, C in ((4, 12), (4, 2056), (0, 64), (-1, 64)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_tome_normalize_f16(x, y, rows, C, st())
    for a, b in ((0, y), (x, 0)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_tome_normalize_f16(a, b, 4, 64, st())
    torch.cuda.synchronize()
    assert R.is_sentinel16(y.cpu())


# ================================================================================================================== row movers
MOVER_C, MOVER_N, MOVER_BT = (8, 320, 1280), (1, 3, 257, 1031), (1, 3)


def strided_in(Bt, rows, C, gap, g):
    """Input [Bt, rows, C] of N(0, 1) values with `gap` sentinel elements between batch entries: -> (flat device buffer, batch stride, CPU values)."""
    v = torch.randn(Bt, rows, C, generator=g).to(H)
    buf = R.sentinel16(Bt, rows * C + gap)
    buf[:, :rows * C] = v.reshape(Bt, -1)
    return dev(buf), rows * C + gap, v


def strided_out(Bt, rows, C, gap):
    return dev(R.sentinel16(Bt, rows * C + gap)), rows * C + gap


def check_out(buf, Bt, rows, C, want, what):
    o = buf.cpu()
    assert eq16(o[:, :rows * C].reshape(Bt, rows, C), want), what
    assert R.is_sentinel16(o[:, rows * C:]), ("gap between batch entries written", what)


@pytest.mark.parametrize("C", MOVER_C)
def test_gather_rows(L, C):
    """map NULL (copy); a map with repeats; a map mixing m >= 0 (row m of s1) and m < 0 (row ~m of s2) with different batch strides of s1 and s2."""
    g = R.rng(C)
    for Bt in MOVER_BT:
        for n in MOVER_N:
            n1, n2 = n + 2, n // 2 + 3
            s1, bs1, v1 = strided_in(Bt, n1, C, 24, g)
            s2, bs2, v2 = strided_in(Bt, n2, C, 56, g)
            pos = torch.randint(0, n1, (n,), generator=g)
            mix = torch.where(torch.rand(n, generator=g) < 0.5, pos, ~torch.randint(0, n2, (n,), generator=g))
            mix[-1] = -1                                    # ~0: the first row of s2
            mix[0] = -n2                                    # ~(n2 - 1): its last row
            for name, m, s2arg, want in (("copy", None, 0, v1[:, :n]), ("repeats", pos, 0, R.gather_rows_ref(v1, None, pos)),
                                         ("two sources", mix, s2, R.gather_rows_ref(v1, v2, mix))):
                out, bso = strided_out(Bt, n, C, 40)
                L.tcl_gather_rows_f16(s1, bs1, s2arg, bs2, dev(m.to(I32)) if m is not None else 0, out, bso, Bt, n, C, st())
                check_out(out, Bt, n, C, want, ("gather_rows", name, C, n, Bt))


@pytest.mark.parametrize("C", MOVER_C)
def test_gather_rows_pair(L, C):
    """Both sets and a single set, map given and NULL."""
    g = R.rng(C + 1)
    for Bt in MOVER_BT:
        for n in MOVER_N:
            ns = n + 3
            sa, bsa, va = strided_in(Bt, ns, C, 24, g)
            sb, bsb, vb = strided_in(Bt, ns, C, 72, g)
            m = torch.randint(0, ns, (n,), generator=g)
            for mp in (m, None):
                wa, wb = (va[:, m], vb[:, m]) if mp is not None else (va[:, :n], vb[:, :n])
                md = dev(mp.to(I32)) if mp is not None else 0
                oa, boa = strided_out(Bt, n, C, 40)
                ob, bob = strided_out(Bt, n, C, 8)
                L.tcl_gather_rows_pair_f16(sa, bsa, sb, bsb, md, oa, boa, ob, bob, Bt, n, C, st())
                check_out(oa, Bt, n, C, wa, ("pair a", C, n, Bt, mp is None))
                check_out(ob, Bt, n, C, wb, ("pair b", C, n, Bt, mp is None))
                oa, boa = strided_out(Bt, n, C, 40)
                L.tcl_gather_rows_pair_f16(sa, bsa, 0, 0, md, oa, boa, 0, 0, Bt, n, C, st())
                check_out(oa, Bt, n, C, wa, ("single set", C, n, Bt, mp is None))


@pytest.mark.parametrize("n", [4 * 2048 * 256 - 1, 4 * 2048 * 256, 4 * 2048 * 256 + 1, 7 * 2048 * 256 + 5])
def test_gather_rows_pair_unrolled_trip(L, n):
    """C = 8 (one 16-byte chunk per row), the grid capped at 2048 blocks of 256, so one grid step is 2048 * 256 chunks.  The unrolled four-in-flight
    trip runs while i + 3 steps < n.  n one below four steps: every thread but the last takes one trip, the last thread a three-step tail instead;
    n equal to four steps: every thread one trip and no tail; n one above: thread 0 a trip and a one-step tail; 7 steps and 5 rows: one trip, then
    a three-step tail, in threads 0..4 a second trip instead.  (The tail loop ALONE runs in test_gather_rows_pair: there the grid is not capped and a thread
    has at most two steps.)"""
    g = R.rng(n)
    C, ns = 8, 1000
    sa, bsa, va = strided_in(1, ns, C, 8, g)
    sb, bsb, vb = strided_in(1, ns, C, 8, g)
    m = torch.randint(0, ns, (n,), generator=g)
    oa, boa = strided_out(1, n, C, 16)
    ob, bob = strided_out(1, n, C, 16)
    L.tcl_gather_rows_pair_f16(sa, bsa, sb, bsb, dev(m.to(I32)), oa, boa, ob, bob, 1, n, C, st())
    check_out(oa, 1, n, C, va[:, m], ("pair a", n))
    check_out(ob, 1, n, C, vb[:, m], ("pair b", n))


@pytest.mark.parametrize("C", MOVER_C)
def test_gather_add_rows(L, C):
    """h = (h + y[map]) with one f32 add and one rounding; the first rows hold sums that round (2048 + 1, 1 + 2^-11: ties to even), +-0 in the four
    sign combinations and a cancellation to +0; the map repeats rows."""
    g = R.rng(C + 2)
    hs = torch.tensor([2048.0, 1.0, -0.0, 0.0, -0.0, 0.0, 3.0, 1e-4], dtype=H)
    ys = torch.tensor([1.0, 2.0 ** -11, 0.0, -0.0, -0.0, 0.0, -3.0, 60000.0], dtype=H)
    for Bt in MOVER_BT:
        for n in MOVER_N:
            ny = n // 2 + 2
            bsh, bsy = n * C + 24, ny * C + 56
            vh = torch.randn(Bt, n, C, generator=g).to(H)
            m = torch.randint(0, ny, (n,), generator=g)
            m[0] = 0
            yv = (torch.randn(Bt, ny, C, generator=g) * 4).to(H)
            vh[:, 0, :8], yv[:, 0, :8] = hs, ys
            hbuf, ybuf = R.sentinel16(Bt, bsh), R.sentinel16(Bt, bsy)
            hbuf[:, :n * C] = vh.reshape(Bt, -1)
            ybuf[:, :ny * C] = yv.reshape(Bt, -1)
            hd = dev(hbuf)
            L.tcl_gather_add_rows_f16(hd, bsh, dev(ybuf), bsy, dev(m.to(I32)), Bt, n, C, st())
            check_out(hd, Bt, n, C, R.gather_add_ref(vh, yv, m), ("gather_add", C, n, Bt))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_index_compose(L, n):
    g = R.rng(n)
    outer = torch.randint(0, 1 << 20, (n + 40,), generator=g).to(I32)
    for off in (0, 7):
        for inner in (None, torch.randint(0, n + 33, (n,), generator=g).to(I32)):
            out = torch.full((n + PAD,), -1, dtype=I32, device="cuda")
            L.tcl_index_compose(dev(outer), dev(inner) if inner is not None else 0, off, n, out, st())
            o = out.cpu()
            assert torch.equal(o[:n], R.index_compose_ref(outer, inner, off, n)), (n, off, inner is None)
            assert (o[n:] == -1).all()


def test_movers_refused_arguments(L):
    h = dev(R.sentinel16(4096))
    i = torch.full((64,), -1, dtype=I32, device="cuda")
    bad = [
        lambda: L.tcl_gather_rows_pair_f16(h, 64, h, 64, 0, h, 64, 0, 64, 1, 4, 8, st()),            # sb without ob
        lambda: L.tcl_gather_rows_pair_f16(h, 64, 0, 64, 0, h, 64, h, 64, 1, 4, 8, st()),            # ob without sb
        lambda: L.tcl_gather_rows_pair_f16(h, 64, 0, 0, 0, h, 64, 0, 0, 1, 4, 12, st()),
        lambda: L.tcl_gather_rows_pair_f16(h, 64, 0, 0, 0, h, 64, 0, 0, 1, 0, 8, st()),
        lambda: L.tcl_gather_rows_pair_f16(0, 64, 0, 0, 0, h, 64, 0, 0, 1, 4, 8, st()),
        lambda: L.tcl_gather_rows_f16(h, 64, 0, 0, 0, h, 64, 1, 4, 12, st()),
        lambda: L.tcl_gather_rows_f16(h, 64, 0, 0, 0, h, 64, 0, 4, 8, st()),
        lambda: L.tcl_gather_rows_f16(h, 64, 0, 0, 0, 0, 64, 1, 4, 8, st()),
        lambda: L.tcl_gather_add_rows_f16(h, 64, h, 64, 0, 1, 4, 4, st()),
        lambda: L.tcl_gather_add_rows_f16(h, 64, 0, 64, 0, 1, 4, 8, st()),
        lambda: L.tcl_gather_add_rows_f16(h, 64, h, 64, 0, 1, 0, 8, st()),
        lambda: L.tcl_index_compose(i, 0, 0, 0, i, st()),
        lambda: L.tcl_index_compose(0, 0, 0, 4, i, st()),
        lambda: L.tcl_index_compose(i, 0, 0, 4, 0, st()),
    ]
    for call in bad:
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            call()
    torch.cuda.synchronize()
    assert R.is_sentinel16(h.cpu()) and (i == -1).all()
