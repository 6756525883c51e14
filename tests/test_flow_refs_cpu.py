"""CPU: the float64 references of tests/flow_refs.py against oracle/ and torch's own convolutions, the lattice claim of the feature maps, the host
restatement of the tile kernel's band decisions, and the float32-against-float64 floors the GPU flow leaf tests take their elementwise atol from."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_refs as R
from oracle import memflow as OM
from tc_light_amd import raft as TR

F64, F32 = torch.float64, torch.float32


def close12(a, b):
    return a.shape == b.shape and (a - b).abs().max().item() <= 1e-12


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def corr_nchw(f1, f2, co, levels, r):
    """corr_ref in float64 on NCHW maps, as [B, L*n*n, H, W]."""
    B, _, Hh, Ww = f1.shape
    out = R.corr_ref(nhwc(f1), [nhwc(g) for g in OM.f2_pyramid(f2.to(F64), levels)], co, r, dt=F64)
    return out.view(B, Hh, Ww, -1).permute(0, 3, 1, 2)


def test_corr_ref_vs_oracle():
    """oracle.memflow.corr_lookup evaluated in float64 (it allocates in the default dtype), r = 4, 4 levels: 1e-12."""
    g = R.rng(1)
    f1, f2 = torch.randn(2, 64, 9, 13, generator=g, dtype=F64), torch.randn(2, 64, 9, 13, generator=g, dtype=F64)
    co = R.grid(2, 9, 13).to(F64) + 3 * torch.randn(2, 2, 9, 13, generator=g, dtype=F64)
    co[:, :, 0, 0] = torch.tensor([-2.5, 3.0], dtype=F64)                 # a negative half-integer and an integer
    torch.set_default_dtype(F64)
    try:
        want = OM.corr_lookup(f1, f2, co)
    finally:
        torch.set_default_dtype(F32)
    assert want.dtype == F64
    assert close12(corr_nchw(f1, f2, co, 4, 4), want)


def test_corr_ref_vs_reference_golden():
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "memflow_corr.npz"))
    for tag in ("a", "b"):
        f1, f2, co, ref = (torch.from_numpy(G[f"{tag}_{k}"]) for k in ("f1", "f2", "coords", "out"))
        got = corr_nchw(f1, f2, co, 4, 4)
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() < 3e-5


def test_lattice_levels_are_exact_in_f16():
    """Every pooled level of every case is on the f16 grid, and pooling in f32 equals pooling in float64: both routes read the same numbers."""
    seen = 0
    for D in R.CORR_D:
        for Hh, Ww, lv in R.CORR_SHAPES:
            _, levels, _ = R.corr_input(D, Hh, Ww, lv, 4, "noise")
            assert len(levels) == lv and tuple(levels[-1].shape[1:3]) == (Hh >> (lv - 1), Ww >> (lv - 1))
            for l, t in enumerate(levels):
                assert torch.equal(t.half().float(), t), (D, Hh, Ww, l)
                if l:
                    assert torch.equal(R.avgpool2_nhwc_ref(levels[l - 1], F64), t.double())
                seen += 1
    for D in R.TILED_D:
        for Hh, Ww in R.TILED_SHAPES:
            for kind in R.TILED_COORDS:
                f1, levels, _ = R.tiled_input(D, Hh, Ww, kind)
                assert torch.equal(f1.half().float(), f1)
                for l, t in enumerate(levels):
                    assert torch.equal(t.half().float(), t), (D, Hh, Ww, kind, l)
                    seen += 1
    assert seen == 4 * (3 + 4 + 4 + 1) + 2 * 3 * 3 * 4
    assert {tuple(R.corr_input(64, h, w, lv, 4, "noise")[1][-1].shape[1:3]) for h, w, lv in R.CORR_SHAPES} == {(1, 1), (2, 3), (4, 4)}


def test_corr_coordinate_sets_are_what_they_claim():
    for Hh, Ww, lv in R.CORR_SHAPES:
        for r in R.CORR_R:
            c = R.corr_coords("integer", 2, Hh, Ww, r, lv, 1)
            assert torch.equal(c, c.round())
            c = R.corr_coords("half", 2, Hh, Ww, r, lv, 1)
            assert torch.equal(c - torch.floor(c), torch.full_like(c, 0.5)) and (c < 0).any()
            c = R.corr_coords("outside", 2, Hh, Ww, r, lv, 1)
            for l in range(lv):                                          # the window [floor - r, floor + r + 1] misses [0, size) by more than r + 1 on one axis
                x, y, Wl, Hl = torch.floor(c[:, 0] / 2 ** l), torch.floor(c[:, 1] / 2 ** l), Ww >> l, Hh >> l
                out = (x + r + 1 < -(r + 1)) | (x - r > Wl - 1 + r + 1) | (y + r + 1 < -(r + 1)) | (y - r > Hl - 1 + r + 1)
                assert out.all(), (Hh, Ww, r, l)
            c = R.corr_coords("border", 2, Hh, Ww, r, lv, 1)
            assert (c[:, 0] - r < 0).any() and (c[:, 0] + r + 1 > Ww - 1).any() and (c[:, 1] - r < 0).any() and (c[:, 1] + r + 1 > Hh - 1).any()


def test_tile_bands_of_the_tiled_coordinate_sets():
    """smooth: one band everywhere; zoom: some tile needs more than one band and none more than CT_MAXB; torn: some but not all flags raised."""
    for D in R.TILED_D[:1]:
        for Hh, Ww in R.TILED_SHAPES:
            for kind in R.TILED_COORDS:
                _, levels, co = R.tiled_input(D, Hh, Ww, kind)
                nb = R.tile_bands(co, [tuple(t.shape[1:3]) for t in levels])
                flagged = int((nb > R.CT_MAXB).sum())
                if kind == "smooth":
                    assert nb.max() == 1 and flagged == 0
                elif kind == "zoom":
                    assert 1 < nb.max() <= R.CT_MAXB
                else:
                    assert 0 < flagged < nb.numel() and nb[0, 0] > R.CT_MAXB
    # one tile by hand: x0 = -4 .. 3 + 9 clipped to [0, 12], y0 likewise to [0, 8] -> 13 x 9 points, one band
    co = R.grid(1, 9, 13)
    assert R.tile_bands(co, [(9, 13)])[0, 0] == 1 and R.tile_bands(co * 0 - 40, [(9, 13)]).max() == 0


# ------------------------------------------------------------------------------------------------------------------ SepConvGRU
def _gru_case(vertical, seed):
    g = R.rng(seed)
    B, Hh, Wd = 2, 3, 7
    shape = (128, 384, 5, 1) if vertical else (128, 384, 1, 5)
    w = {k: torch.randn(*shape, generator=g, dtype=F64) / 1920 ** 0.5 for k in "zrq"}
    b = {k: torch.randn(128, generator=g, dtype=F64) for k in "zrq"}
    h, inp, mot = (torch.randn(B, 128, Hh, Wd, generator=g, dtype=F64) for _ in range(3))
    return B, Hh, Wd, w, b, h, inp, mot


@pytest.mark.parametrize("vertical", [0, 1])
def test_sepconv_refs_vs_conv2d(vertical):
    """One SepConvGRU half (update.py:43-56) with F.conv2d on NCHW against fold / gate / cand on rows with the engine's weight layout."""
    B, Hh, Wd, w, b, h, inp, mot = _gru_case(vertical, 7 + vertical)
    pad = (2, 0) if vertical else (0, 2)
    hx = torch.cat([h, inp, mot], 1)
    z = torch.sigmoid(F.conv2d(hx, w["z"], b["z"], padding=pad))
    r = torch.sigmoid(F.conv2d(hx, w["r"], b["r"], padding=pad))
    q = torch.tanh(F.conv2d(torch.cat([r * h, inp, mot], 1), w["q"], b["q"], padding=pad))
    h_new = (1 - z) * h + z * q
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * Hh * Wd, -1)
    zr, tq = torch.cat([TR.gru_taps(w["z"]), TR.gru_taps(w["r"])]), TR.gru_taps(w["q"])
    w_zr, w_q, c_zr, c_q = TR.gru_hm_weight(zr), TR.gru_hm_weight(tq), TR.gru_ctx_weight(zr), TR.gru_ctx_weight(tq)
    assert w_zr.shape == (256, 1280) and c_q.shape == (128, 640)
    assert w_zr[130, 3 * 256 + 128 + 5] == w["r"].reshape(128, 384, 5)[2, 256 + 5, 3]          # column tap*256 + src*128 + c
    pb_zr = R.fold_ref(rows(inp), None, c_zr, torch.cat([b["z"], b["r"]]), Hh, Wd, vertical, dt=F64)
    pb_q = R.fold_ref(rows(inp), None, c_q, b["q"], Hh, Wd, vertical, dt=F64)
    gz, grh = R.gate_ref(rows(h), rows(mot), w_zr, pb_zr, Hh, Wd, vertical, dt=F64)
    assert close12(gz, rows(z)) and close12(grh, rows(r * h))
    got = R.cand_ref(grh, rows(mot), w_q, pb_q, gz, rows(h), Hh, Wd, vertical, dt=F64)
    assert close12(got, rows(h_new))
    # the plain convolution, both source counts
    assert close12(R.sepconv_ref(rows(inp), None, c_q, Hh, Wd, vertical, dt=F64), rows(F.conv2d(inp, w["q"][:, 128:256], None, padding=pad)))
    assert close12(R.sepconv_ref(rows(h), rows(mot), w_q, Hh, Wd, vertical, dt=F64),
                   rows(F.conv2d(torch.cat([h, mot], 1), torch.cat([w["q"][:, :128], w["q"][:, 256:]], 1), None, padding=pad)))
    # layout mutations must be visible: the tap order reversed, the two sources swapped
    flipped = w_zr.view(256, 5, 256).flip(1).reshape(256, 1280)
    assert not close12(R.gate_ref(rows(h), rows(mot), flipped, pb_zr, Hh, Wd, vertical, dt=F64)[0], rows(z))
    assert not close12(R.gate_ref(rows(mot), rows(h), w_zr, pb_zr, Hh, Wd, vertical, dt=F64)[0], rows(z))
    # and the other direction is another operation
    assert not close12(R.gate_ref(rows(h), rows(mot), w_zr, pb_zr, Hh, Wd, 1 - vertical, dt=F64)[0], rows(z))


def test_sepconv_ref_short_axis_and_batch_boundary():
    """(1,1,4) vertical: only the centre tap is inside.  (2,3,7): nothing crosses from one image into the next."""
    i = R.sep_input(1, 1, 4, 128, 0, 3)
    centre = i["s0"].double() @ i["w"].double().view(128, 5, 128)[:, 2].t()
    assert close12(R.sepconv_ref(i["s0"], None, i["w"], 1, 4, 1, dt=F64), centre)
    i = R.sep_input(2, 3, 7, 128, 128, 4)
    for vertical in (0, 1):
        both = R.sepconv_ref(i["s0"], i["s1"], i["w"], 3, 7, vertical, dt=F64)
        for b in range(2):
            one = R.sepconv_ref(i["s0"][21 * b:21 * b + 21], i["s1"][21 * b:21 * b + 21], i["w"], 3, 7, vertical, dt=F64)
            assert torch.equal(both[21 * b:21 * b + 21], one)


def test_convf1_ref_vs_conv2d():
    g = R.rng(9)
    B, Hh, Ww = 2, 5, 9
    w, b = torch.randn(128, 2, 7, 7, generator=g, dtype=F64) / 7, torch.randn(128, generator=g, dtype=F64)
    c0 = R.grid(B, Hh, Ww)
    c1 = c0 + 3 * torch.randn(B, 2, Hh, Ww, generator=g)
    w_t = TR.convf1_weight_t(w)
    assert w_t.shape == (98, 128) and w_t[1 * 49 + 2 * 7 + 3, 5] == w[5, 1, 2, 3]
    want = torch.relu(F.conv2d((c1 - c0).to(F64), w, b, padding=3)).permute(0, 2, 3, 1).reshape(B * Hh * Ww, 128)
    assert close12(R.convf1_ref(c1, w_t, b, dt=F64), want)
    _, wt2, _ = R.convf1_input(1, 3, 5, "noise")                         # the inputs of the GPU cases use the engine's transposition
    assert torch.equal(wt2, TR.convf1_weight_t(wt2.t().reshape(128, 2, 7, 7)))
    far = R.convf1_input(2, 7, 11, "far")[0] - R.grid(2, 7, 11)
    assert far.abs().max() > 300 and far.abs().max() <= 400


# ------------------------------------------------------------------------------------------------------------------ floors
_CASES = list(R.f16_floor_cases())


def test_every_f16_output_has_floor_cases():
    assert {c[0] for c in _CASES} == {"corr_rows", "corr_tiled", "sepconv_gate", "sepconv_cand", "convf1"}
    assert len({(c[0], c[1]) for c in _CASES}) == len(_CASES)


@pytest.mark.parametrize("kernel", sorted({c[0] for c in _CASES}))
def test_f16_floor_is_small_against_the_output(kernel):
    """atol = 4 x max|float32 - float64| stays under ATOL_CAP of the output's RMS (an all-zero output has atol 0).  The bound is relative only: the
    convf1 outputs of the few-hundred-pixel flows are of order 100."""
    worst, worst_rel = 0.0, 0.0
    for name, cid, fn, args in _CASES:
        if name != kernel:
            continue
        atol, rms = R.atol_of(name, cid)
        assert (atol, rms) == R.floor_atol(fn, *args)                       # what the GPU tests import is what is pinned here
        assert atol <= R.ATOL_CAP * rms, (name, cid, atol, rms)
        worst, worst_rel = max(worst, atol), max(worst_rel, atol / rms if rms else 0.0)
    print(f"[flow leaf floor] {kernel}: largest atol {worst:.3e}, largest atol / rms {worst_rel:.3e}")
