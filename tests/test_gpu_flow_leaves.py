"""GPU: leaf parity of the kernels inside every iteration of both flow estimators -- k_corr_lookup, k_corr_lookup_tile (csrc/flow.hip), k_sepconv,
k_convf1 (csrc/raft.hip) -- each through the C ABI against a float64 evaluation of the same operation on the kernel's own rounded inputs
(tests/flow_refs.py, pinned by tests/test_flow_refs_cpu.py).

Assertion classes (tests/leaf_refs.py):
  f16 output  rel-L2 <= 2e-3 and, elementwise, |got - ref| <= 2^-10 |ref| + atol with atol = 4 x max|float32 - float64| of the same operation on the same
              inputs.  Largest atol per kernel: corr_lookup_rows 1.2e-5, corr_lookup_tiled 8.8e-6, sepconv gate (r*h) 7.3e-7,
              sepconv candidate (h) 2.2e-6, convf1 1.2e-5 at flows of a few pixels and 1.5e-3 at flows of a few hundred (outputs of order 100).
  f32 output  |got - ref| <= 3e-5 max(1, max|ref|).
  exact       windows wholly outside the map give 0; refused calls, padding columns and guard rows keep their bits.
Feature maps lie on the lattice k/8, |k| <= 32, so the f32 pyramid of the per-pixel route and the f16 pyramid of the tiled route hold the same numbers and
one reference serves both.  Rows sit inside larger buffers with sentinel (f16) or NaN (f32) guard rows before row 0 and after row M - 1: a read outside
[0, M) poisons the result, a write outside is seen by the bit compare.  Every check prints its figures (`-s`); profiles/flow_leaf_parity.txt keeps one run's."""
import ctypes

import pytest
import torch

import flow_refs as R

pytestmark = pytest.mark.gpu
H, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float("nan")
GUARD = 40                    # guard rows: more than the 2 * W = 32 rows a vertical tap of the widest case reaches


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
    return t.contiguous().view(torch.int16 if t.dtype == H else torch.int32)


class Guarded:
    """Rows [M, C] in the middle of a [GUARD + M + GUARD, C] device buffer whose other rows hold the f16 sentinel / NaN; `fill` None: the middle too."""

    def __init__(self, M, C, dtype, fill=None):
        buf = R.sentinel16(2 * GUARD + M, C) if dtype == H else torch.full((2 * GUARD + M, C), NAN, dtype=F32)
        if fill is not None:
            buf[GUARD:GUARD + M] = fill
        self.buf, self.M = buf.cuda(), M
        self.mid = self.buf[GUARD:GUARD + M]
        self.before = self.buf.clone()

    def guards_intact(self):
        return torch.equal(bits(self.buf[:GUARD]), bits(self.before[:GUARD])) and torch.equal(bits(self.buf[GUARD + self.M:]), bits(self.before[GUARD + self.M:]))

    def untouched(self):
        return torch.equal(bits(self.buf), bits(self.before))


def check_f16(name, case, got, ref, atol):
    """The two assertions of an f16-output kernel; got on the device, ref float64 on the CPU."""
    got = got.cpu()
    assert got.shape == ref.shape
    rel, ex = R.rel_l2(got, ref), R.elem_excess(got, ref, atol)
    print(f"[flow leaf] {name} {case}: rel-L2 {rel:.2e}  elementwise {ex:.3f} of (2^-10 |ref| + {atol:.2e})")
    assert not torch.isnan(got.float()).any(), (name, case)
    assert rel <= R.REL_F16, (name, case, rel)
    assert ex <= 1.0, (name, case, ex)


def check_f32(name, case, got, ref):
    got = got.cpu().double()
    assert got.shape == ref.shape
    tol, err = R.f32_tol(ref), (got - ref).abs().max().item()
    print(f"[flow leaf] {name} {case}: max|got - ref| {err:.2e}  (tolerance {tol:.2e})")
    assert not torch.isnan(got).any(), (name, case)
    assert err <= tol, (name, case, err, tol)


def refused(fn, *args):
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        fn(*args)
    torch.cuda.synchronize()


# ================================================================================================================== correlation lookup
class Maps:
    """f1 and the fmap2 pyramid on the device (f32, and f16 for the tiled entry) with the pointer / size arrays of the C ABI.  An entry count of 1 reads
    the first entry of the same buffers."""

    def __init__(self, f1, levels):
        n = len(levels)
        self.f1, self.lv = dev(f1), [dev(t) for t in levels]
        self.f1h, self.lvh = self.f1.half(), [t.half() for t in self.lv]
        self.ptr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.lv])
        self.ptrh = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.lvh])
        self.hs = (ctypes.c_int * n)(*[t.shape[1] for t in levels])
        self.ws = (ctypes.c_int * n)(*[t.shape[2] for t in levels])
        self.n = n


@pytest.mark.parametrize("Hh,Ww,lv", R.CORR_SHAPES)
@pytest.mark.parametrize("D", R.CORR_D)
def test_corr_lookup_f32(L, D, Hh, Ww, lv):
    """The per-pixel kernel, f32 out: both feature layouts (D % 256), r = 1 / 4 / 5, 1 and 2 entries, both output layouts, five coordinate sets."""
    P, maps = Hh * Ww, None
    for r in R.CORR_R:
        C = lv * (2 * r + 1) ** 2
        for kind in R.CORR_COORDS:
            f1, levels, co = R.corr_input(D, Hh, Ww, lv, r, kind)
            maps = maps or Maps(f1, levels)                              # the maps do not depend on r or on the coordinate set
            ref, cod = R.corr_ref(f1, levels, co, r, dt=F64), dev(co[:1])
            cod2 = dev(co)
            for B in R.CORR_B:
                for nchw in (0, 1):
                    out = torch.full((B * P * C + 64,), NAN, dtype=F32, device="cuda")
                    L.tcl_corr_lookup_f32(maps.f1, maps.ptr, maps.hs, maps.ws, lv, cod if B == 1 else cod2, out, B, Hh, Ww, D, r, nchw, st())
                    got = out[:B * P * C].view(B, C, P).transpose(1, 2) if nchw else out[:B * P * C].view(B, P, C)
                    check_f32("corr_lookup_f32", (D, Hh, Ww, lv, r, kind, B, nchw), got, ref[:B])
                    assert torch.isnan(out[B * P * C:]).all()
                    if kind == "outside":
                        assert (got == 0).all()


@pytest.mark.parametrize("Hh,Ww,lv", R.CORR_SHAPES)
@pytest.mark.parametrize("D", R.ROWS_D)
def test_corr_lookup_rows_f16(L, D, Hh, Ww, lv):
    """The same kernel writing f16 rows [2 P, ld]: ld = 384 and ld = L n^2; padding columns and guard rows keep the sentinel."""
    P, maps = Hh * Ww, None
    for r in R.ROWS_R:
        C = lv * (2 * r + 1) ** 2
        for kind in R.CORR_COORDS:
            f1, levels, co = R.corr_input(D, Hh, Ww, lv, r, kind)
            maps = maps or Maps(f1, levels)
            ref, cod, atol = R.corr_ref(f1, levels, co, r, dt=F64).reshape(2 * P, C), dev(co), R.atol_of("corr_rows", (D, Hh, Ww, lv, r, kind))[0]
            for ld in (384, C):
                rows = Guarded(2 * P, ld, H)
                L.tcl_corr_lookup_rows_f16(maps.f1, maps.ptr, maps.hs, maps.ws, lv, cod, rows.mid, ld, 2, Hh, Ww, D, r, st())
                check_f16("corr_lookup_rows_f16", (D, Hh, Ww, lv, r, kind, ld), rows.mid[:, :C], ref, atol)
                assert torch.equal(bits(rows.mid[:, C:]), bits(rows.before[GUARD:GUARD + 2 * P, C:])) and rows.guards_intact()
                if kind == "outside":
                    assert (rows.mid[:, :C] == 0).all()


@pytest.mark.parametrize("Hh,Ww", R.TILED_SHAPES)
@pytest.mark.parametrize("D", R.TILED_D)
def test_corr_lookup_tiled(L, D, Hh, Ww):
    """The tile-sharing kernel against corr_ref on its f16 levels (not against the other kernel): smooth -- no flag; zoom -- more than one staging band,
    no flag; torn -- some tiles flagged and served by the per-pixel kernel inside the same call, bit-identical to tcl_corr_lookup_rows_f16 there.  The
    flags equal the host restatement of the kernel's band decision."""
    P, tx, ty = Hh * Ww, (Ww + 7) // 8, (Hh + 7) // 8
    for kind in R.TILED_COORDS:
        f1, levels, co = R.tiled_input(D, Hh, Ww, kind)
        maps, cod = Maps(f1, levels), dev(co)
        assert all(torch.equal(a.float(), b) for a, b in zip(maps.lvh, maps.lv))
        ref = R.corr_ref(f1.half(), [t.half() for t in levels], co, 4, dt=F64)[0]
        rows, flags = Guarded(P, 384, H), torch.full((4 * tx * ty,), -1, dtype=torch.int32, device="cuda")
        L.tcl_corr_lookup_rows_tiled_f16(maps.f1h, maps.ptrh, maps.f1, maps.ptr, maps.hs, maps.ws, 4, cod, rows.mid, 384, Hh, Ww, D, 4, flags, st())
        bands = R.tile_bands(co, [tuple(t.shape[1:3]) for t in levels])
        fl = flags.cpu().view(4, ty * tx)
        nf = int(fl.sum())
        print(f"[flow leaf] corr_lookup_tiled {(D, Hh, Ww, kind)}: flags {nf} / {fl.numel()}, most bands {int(bands[bands <= R.CT_MAXB].max())}")
        assert torch.equal(fl.long(), (bands > R.CT_MAXB).long())
        if kind == "smooth":
            assert nf == 0
        elif kind == "zoom":
            assert nf == 0 and bands.max() > 1
        else:
            assert 0 < nf < fl.numel() and fl[0].any()
        check_f16("corr_lookup_tiled", (D, Hh, Ww, kind), rows.mid[:, :324], ref, R.atol_of("corr_tiled", (D, Hh, Ww, kind))[0])
        assert torch.equal(bits(rows.mid[:, 324:]), bits(rows.before[GUARD:GUARD + P, 324:])) and rows.guards_intact()
        if kind == "torn":
            pp = Guarded(P, 384, H)
            L.tcl_corr_lookup_rows_f16(maps.f1, maps.ptr, maps.hs, maps.ws, 4, cod, pp.mid, 384, 1, Hh, Ww, D, 4, st())
            p = torch.arange(P)
            tile_of = ((p // Ww) // 8) * tx + (p % Ww) // 8
            for l in range(4):
                m = fl[l].bool()[tile_of].cuda()
                if m.any():
                    assert torch.equal(bits(rows.mid[m][:, 81 * l:81 * l + 81]), bits(pp.mid[m][:, 81 * l:81 * l + 81])), l


# ================================================================================================================== SepConvGRU half-steps
@pytest.mark.parametrize("vertical", [0, 1])
@pytest.mark.parametrize("B,Hh,Wd", R.SEP_SHAPES)
def test_raft_sepconv(L, B, Hh, Wd, vertical):
    """The three epilogues at whole tiles (M = 256), a one-row tail tile (65), less than a tile with a batch boundary and an axis shorter than the taps
    (42), batch boundaries beside the tile boundaries (189) and a single image row (4)."""
    M = B * Hh * Wd
    for name, mode, N, C1 in R.SEP_CONFIGS:
        i, fn, args = R.sep_case(name, N, C1, B, Hh, Wd, vertical)
        case = (name, N, C1, B, Hh, Wd, vertical)
        s0, w = Guarded(M, 128, H, i["s0"]), dev(i["w"])
        s1 = Guarded(M, 128, H, i["s1"]) if C1 else None
        s1p = s1.mid if C1 else 0
        ins = [s0] + ([s1] if C1 else [])
        if mode == 0:
            out = Guarded(M, N, F32)
            L.tcl_raft_sepconv_f16(s0.mid, s1p, C1, w, dev(i["bias"]), 0, out.mid, 0, 0, 0, B, Hh, Wd, N, vertical, 0, st())
            check_f32("sepconv fold", case, out.mid, fn(*args, dt=F64))
            outs = [out]
        elif mode == 1:                                                   # src0 is h itself, as the engine calls it
            h, pb, z, rh = Guarded(M, 128, H, i["h"]), Guarded(M, 256, F32, i["pb"]), Guarded(M, 128, F32), Guarded(M, 128, H)
            L.tcl_raft_sepconv_f16(h.mid, s1p, 128, w, 0, pb.mid, 0, z.mid, rh.mid, h.mid, B, Hh, Wd, 256, vertical, 1, st())
            z_ref, rh_ref = R.gate_ref(i["h"], i["s1"], i["w"], i["pb"], Hh, Wd, vertical, dt=F64)
            check_f32("sepconv gate z", case, z.mid, z_ref)
            check_f16("sepconv gate r*h", case, rh.mid, rh_ref, R.atol_of("sepconv_gate", (B, Hh, Wd, vertical))[0])
            ins, outs = [s1, h, pb], [z, rh]
        else:
            h, pb, z = Guarded(M, 128, H, i["h"]), Guarded(M, 128, F32, i["pb"]), Guarded(M, 128, F32, i["z"])
            L.tcl_raft_sepconv_f16(s0.mid, s1p, 128, w, 0, pb.mid, 0, z.mid, 0, h.mid, B, Hh, Wd, 128, vertical, 2, st())
            check_f16("sepconv candidate h", case, h.mid, fn(*args, dt=F64), R.atol_of("sepconv_cand", (B, Hh, Wd, vertical))[0])
            ins, outs = ins + [pb, z], [h]
        assert all(t.untouched() for t in ins), case
        assert all(t.guards_intact() for t in outs), case


# ================================================================================================================== convf1
@pytest.mark.parametrize("B,Hh,Ww,ldo", R.CONVF1_CASES)
def test_raft_convf1(L, B, Hh, Ww, ldo):
    """Every window clipped (3x5), a 26-pixel tail block with ldo = 136 (padding columns keep the sentinel), one whole block; flows of a few pixels and
    of a few hundred."""
    M = B * Hh * Ww
    for kind in R.CONVF1_COORDS:
        c1, w_t, b = R.convf1_input(B, Hh, Ww, kind)
        y = Guarded(M, ldo, H)
        L.tcl_raft_convf1_f16(dev(c1), dev(w_t), dev(b), y.mid, ldo, B, Hh, Ww, st())
        check_f16("convf1", (B, Hh, Ww, ldo, kind), y.mid[:, :128], R.convf1_ref(c1, w_t, b, dt=F64), R.atol_of("convf1", (B, Hh, Ww, kind))[0])
        assert torch.equal(bits(y.mid[:, 128:]), bits(y.before[GUARD:GUARD + M, 128:])) and y.guards_intact()


# ================================================================================================================== refusals
def test_refusals_launch_nothing(L):
    """Unsupported shapes return TCL_EINVAL before any launch: every output keeps its prefill."""
    B, Hh, Wd = 1, 5, 13
    M = B * Hh * Wd
    i = R.sep_input(B, Hh, Wd, 256, 128, 1)
    s0, s1, w, bias, pb = dev(i["s0"]), dev(i["s1"]), dev(i["w"]), dev(i["bias"]), dev(i["pb"])
    o32, z, rh, h = Guarded(M, 256, F32), Guarded(M, 128, F32), Guarded(M, 128, H), Guarded(M, 128, H)
    sep = L.tcl_raft_sepconv_f16
    refused(sep, s0, 0, 0, w, bias, 0, o32.mid, 0, 0, 0, B, Hh, Wd, 192, 0, 0, st())                       # N = 192
    refused(sep, s0, s1, 128, w, 0, pb, 0, z.mid, rh.mid, h.mid, B, Hh, Wd, 128, 0, 1, st())               # mode 1 with N = 128
    refused(sep, s0, s1, 128, w, bias, pb, o32.mid, z.mid, rh.mid, h.mid, B, Hh, Wd, 128, 0, 3, st())      # mode 3
    refused(sep, s0, s1, 64, w, bias, 0, o32.mid, 0, 0, 0, B, Hh, Wd, 128, 0, 0, st())                     # C1 = 64
    refused(sep, s0, 0, 128, w, bias, 0, o32.mid, 0, 0, 0, B, Hh, Wd, 128, 0, 0, st())                     # C1 = 128 without src1
    assert all(t.untouched() for t in (o32, z, rh, h))

    Hc, Wc = 9, 13
    P = Hc * Wc
    f1, levels, co = R.corr_input(64, Hc, Wc, 4, 4, "noise")
    maps, cod = Maps(f1, levels), dev(co)
    f96 = Maps(torch.zeros(2, Hc, Wc, 96), [torch.zeros(2, Hc >> l, Wc >> l, 96) for l in range(4)])
    lv5 = Maps(f1, levels + levels[-1:])
    o = Guarded(2 * P, 5 * 169, F32)
    rows, flags = Guarded(2 * P, 5 * 169, H), torch.full((4 * 4,), -1, dtype=torch.int32, device="cuda")
    for m, nl, D, r in ((f96, 4, 96, 4), (maps, 4, 64, 6), (lv5, 5, 64, 4)):                                  # D = 96, r = 6, 5 levels
        refused(L.tcl_corr_lookup_f32, m.f1, m.ptr, m.hs, m.ws, nl, cod, o.mid, 2, Hc, Wc, D, r, 0, st())
        refused(L.tcl_corr_lookup_rows_f16, m.f1, m.ptr, m.hs, m.ws, nl, cod, rows.mid, 5 * 169, 2, Hc, Wc, D, r, st())
    refused(L.tcl_corr_lookup_rows_tiled_f16, maps.f1h, maps.ptrh, maps.f1, maps.ptr, maps.hs, maps.ws, 4, cod, rows.mid, 5 * 169, Hc, Wc, 64, 3, flags, st())
    assert o.untouched() and rows.untouched() and (flags == -1).all()

    c1, w_t, b = R.convf1_input(1, 3, 5, "noise")
    y = Guarded(15, 136, H)
    for ldo in (120, 132):
        refused(L.tcl_raft_convf1_f16, dev(c1), dev(w_t), dev(b), y.mid, ldo, 1, 3, 5, st())
    assert y.untouched()
