"""CPU: the float64 references of tests/elem_refs.py against the torch function of the same name (and oracle/scheduler.py for the use of the DPM
coefficients), the case tables against the branches they are meant to reach, and the float32-against-float64 floors the GPU leaf tests of
csrc/elem.hip take their elementwise atol from.  A wrong reference or a loose floor then cannot pass quietly."""
import math

import pytest
import torch
import torch.nn.functional as F

import elem_refs as R

F64, F32, H = torch.float64, torch.float32, torch.float16


def close9(a, b):
    return (a - b).abs().max().item() <= 1e-9


@pytest.mark.parametrize("case", [((3, 690, 320, 0, 32), "off4", 1), ((2, 150, 328, 312, 32), "std", 1), ((1, 33, 64, 0, 1), "std", 1), ((1, 33, 512, 0, 64), "std", 1)])
def test_groupnorm_refs_vs_torch(case):
    """Both forms -- the two-pass reference and the one-pass form the floor is taken from -- equal F.group_norm in float64 to 1e-9, offset 4 included."""
    shape, kind, gscale = case
    x1, x2, ga, be = R.gn_input(shape, kind, gscale)
    x = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], -1)
    want = F.group_norm(x.permute(0, 2, 1), shape[4], ga.double(), be.double(), R.EPS_GN).permute(0, 2, 1)
    for silu in (0, 1):
        w = F.silu(want) if silu else want
        assert close9(R.groupnorm_two_pass_ref(x1, x2, ga, be, shape[4], R.EPS_GN, silu), w)
        assert close9(R.groupnorm_ref(x1, x2, ga, be, shape[4], R.EPS_GN, silu, dt=F64), w)


def test_groupnorm_tables_reach_their_branches():
    shapes = {s for s, _, _ in R.GN_CASES}
    assert {(c1 + c2) // g for _, _, c1, c2, g in shapes} >= {4, 6, 7, 10, 20, 30, 80, 8, 64, 40}
    assert any((c1 + c2) // 8 > 256 for _, _, c1, c2, _ in shapes)                                   # the second channel window
    assert any(c2 and c1 % ((c1 + c2) // g) for _, _, c1, c2, g in shapes)                           # a concat seam inside a group
    blocks = lambda hw: -(-hw // -(-hw // min(-(-hw // 64), 256)))                                   # the row partition of tcl_groupnorm_concat_f16
    assert blocks(4099) == 65 and 4099 - 64 * 64 == 3 and -(-16411 // 64) > 256 and blocks(16411) >= 8 * 31
    for _, hw, c1, c2, g in shapes:
        assert not R.gn_chunk_spans_three_groups(c1 + c2, g)
        assert hw <= 1024 or all(k == "std" for s, k, _ in R.GN_CASES if s[1] == hw)                 # offset 4 only at HW <= 1024
    B, HW, C1, C2, G = R.GN_REFUSED
    assert R.gn_chunk_spans_three_groups(C1 + C2, G) and (8 + 7) // 5 - 8 // 5 == 2
    # of the channel counts per group the entry admits (>= 4), 5 is the only one with such a chunk
    for cpg in range(4, 41):
        for G in (1, 2, 32, 64):
            if (cpg * G) % 8 == 0:
                assert R.gn_chunk_spans_three_groups(cpg * G, G) == (cpg == 5), (cpg, G)


def test_group_excess_sees_one_group():
    ref = torch.ones(2, 3, 16, dtype=F64)
    got = ref.clone()
    got[1, :, 4:8] += 0.01
    q = R.group_excess(got, ref, 0.0, 4)
    assert q.shape == (2, 4) and q[1, 1] > 1 and (q.flatten()[[0, 1, 2, 3, 4, 6, 7]] == 0).all()


def test_layernorm_ref_vs_torch():
    for C, rows, kind in ((520, 17, "std"), (640, 17, "off4"), (1544, 17, "const"), (8, 1, "std")):
        x, ga, be = R.ln_input(C, rows, kind)
        got = R.layernorm_ref(x, ga, be, R.EPS_LN, dt=F64)
        assert close9(got, F.layer_norm(x.double(), (C,), ga.double(), be.double(), R.EPS_LN))
        if kind == "const":
            assert torch.equal(got[R.LN_CONST_ROW], be.double())
    assert {(C // 8 + 63) // 64 for C in R.LN_C} == {1, 2, 3, 4} and {(C // 8) % 64 for C in R.LN_C} >= {1}


def test_softmax_ref_and_forms():
    for T, ld, form in R.SOFTMAX_CASES:
        assert R.softmax_form(T, ld) == form and ld >= T
    for kind in R.SOFTMAX_KINDS:
        x = R.softmax_input(1001, kind)
        s32 = torch.tensor(R.SOFTMAX_SCALE, dtype=F32).double()
        assert close9(R.softmax_ref(x, R.SOFTMAX_SCALE, dt=F64), torch.softmax(x.double() * s32, -1))
    e = R.softmax_ref(R.softmax_input(1001, "spike"), R.SOFTMAX_SCALE, dt=F64)
    for r, col in enumerate((715, 0, 1000)):
        others = torch.cat([e[r, :col], e[r, col + 1:]])
        assert e[r].argmax() == col and others.max() < 2.0 ** -14 and (others.half() == 0).any()       # subnormal or zero as f16
    assert torch.allclose(R.softmax_ref(R.softmax_input(1001, "equal"), R.SOFTMAX_SCALE, dt=F64), torch.full((3, 1001), 1 / 1001, dtype=F64), rtol=1e-12)
    lo = R.softmax_input(1001, "min")
    assert (lo == -65504).sum() == 3 and R.softmax_ref(lo, R.SOFTMAX_SCALE, dt=F64)[0, 715] == 0


def test_geglu_gemv_temb_refs():
    x = R.geglu_input(1280, 500)
    assert close9(R.geglu_ref(x, dt=F64), x[:, :1280].double() * F.gelu(x[:, 1280:].double()))
    assert x[0, 1280:].float().min() == -12 and x[0, 1280:].float().max() == 12
    for N, K, fl in R.GEMV_CASES:
        W, v, b, a = R.gemv_input(N, K, fl)
        xv = F.silu(v.double()).half().double() if fl[0] else v.double()
        s = W.double() @ xv + (b.double() if fl[2] else 0)
        s = F.silu(s) if fl[1] else s
        want = s.half().double() + a.double() if fl[3] else s
        assert close9(R.gemv_ref(W, v, b if fl[2] else None, a if fl[3] else None, fl[0], fl[1], dt=F64), want)
        if fl[0]:                  # the float32 SiLU rounds to the same f16 vector: the reference has one vector to multiply
            assert torch.equal(F.silu(v.float()).half(), F.silu(v.double()).half())
        if fl[3]:
            amb, alt = R.gemv_alt_ref(W, v, b, a, fl[0], fl[1], R.atol_of("gemv_presum", (N, K, fl))[0])
            print(f"[elem floor] gemv {N}x{K}: {int(amb.sum())} of {N} sums within the float32 floor of an f16 rounding tie")
            assert amb.float().mean() < 0.05 and ((alt - want).abs() <= 2.0 ** -10 * s.abs() + 2.0 ** -24).all()
    assert {fl for _, _, fl in R.GEMV_CASES} >= {(0, 1, True, False), (0, 0, True, False), (1, 0, True, True)}       # UNetEngine._temb
    fr = torch.exp(-math.log(10000.0) * torch.arange(160, dtype=F64) / 160)
    assert close9(R.timestep_embed_ref(801.0, 320, dt=F64), torch.cat([torch.cos(801.0 * fr), torch.sin(801.0 * fr)]))


def test_unpack_cfg_ref_vs_test_formula():
    """The yt case against the einsum-free formula of test_pack_unpack_adain (tests/test_gpu_kernels.py), and the bytes each mode leaves alone."""
    case = R.UNPACK_CASES[1]
    name, mode, idx, sl, nwin, guidance, scale_upto, scale, nkeep = case
    eps = R.unpack_input(case)
    out, mask = R.unpack_cfg_ref(eps, case, dt=F64)
    e = eps.double().permute(0, 3, 1, 2)                                   # [2F, c, n, h]
    pred = e[:4] + guidance * (e[4:] - e[:4])                              # w c n h
    want = torch.zeros(R.UNPACK_N, 4, R.UNPACK_H, R.UNPACK_W, dtype=F64)
    want[sl:sl + nwin][:, :, :, list(idx)] = pred.permute(2, 1, 3, 0)
    want[sl:scale_upto] *= torch.tensor(scale, dtype=F32).double()
    want[sl + nkeep:] = 0
    assert close9(out, want)
    cols = torch.zeros(R.UNPACK_W, dtype=torch.bool)
    cols[list(idx)] = True
    assert mask[sl:sl + nkeep][:, :, :, cols].all() and not mask[sl:sl + nkeep][:, :, :, ~cols].any() and not mask[:sl].any() and not mask[sl + nkeep:].any()
    assert nkeep < nwin and sl < scale_upto < sl + nkeep and list(idx) != sorted(idx) and R.UNPACK_H != R.UNPACK_W
    out0, mask0 = R.unpack_cfg_ref(R.unpack_input(R.UNPACK_CASES[0]), R.UNPACK_CASES[0], dt=F64)
    assert mask0[[5, 1, 2]].all() and not mask0[[0, 3, 4, 6]].any()


def test_adain_ref_vs_test_formula():
    """The formula of test_pack_unpack_adain (tests/test_gpu_kernels.py) in float64."""
    for hw in R.ADAIN_HW:
        a, b = R.adain_input(hw)
        a0, b0 = a.double(), b.double()
        ms = lambda t: (t.mean(1, keepdim=True), (t.var(1, keepdim=True) + 1e-5).sqrt())
        (ma, sa), (mb, sb) = ms(a0), ms(b0)
        ra = (a0 - ma) / sa * sb + mb
        assert close9(R.adain_first_ref(a, b, dt=F64), ra)
        al = torch.tensor(R.ADAIN_ALPHA, dtype=F32).double()
        assert close9(R.adain_second_ref(ra.half(), b, R.ADAIN_ALPHA, dt=F64), al.sqrt() * ra.half().double() + (1 - al).sqrt() * b0)
        assert abs(a0.mean().item() - 3) < 0.2 and abs(a0.std().item() - 0.2) < 0.1
    assert any(hw % 256 for hw in R.ADAIN_HW) and 2 in R.ADAIN_HW


def test_dpm_ref_vs_oracle_scheduler():
    """The kernel's expression with tc_light_amd.scheduler's coefficients for two real consecutive steps (the 20-step schedule entered at index 15: order 1,
    then order 2) against oracle/scheduler.py stepping from the same index.  The oracle evaluates in float32 with its own float32 coefficient
    arithmetic, so the pin is 1e-5 of the largest value, not 1e-9."""
    from oracle.scheduler import Scheduler as OS
    g = R.rng(5)
    n = 257
    x = torch.randn(n, generator=g).half()
    e1, z1, e2, z2 = (torch.randn(n, generator=g).half() for _ in range(4))
    c1, c2 = R.dpm_coefficients(False), R.dpm_coefficients(True)
    for c in (c1, c2):
        assert c[0] / c[1] <= 0.25                                        # sigma_t / alpha_t: the premise of the f32 bound (elem_refs docstring)
    assert c1[4] == 0.0 and c2[4] != 0.0
    m0a = R.dpm_m0_ref(x, e1, c1, dt=F64)
    xa = R.dpm_x_ref(x, e1, None, z1, c1, dt=F64)
    xb = R.dpm_x_ref(xa, e2, m0a, z2, c2, dt=F64)
    osch = OS(R.DPM_STEPS)
    osch.i = R.DPM_BEGIN
    oa = osch.step(e1, x, z1)
    ob = osch.step(e2, oa, z2)
    assert (xa - oa.double()).abs().max() <= 1e-5 * xa.abs().max() and (xb - ob.double()).abs().max() <= 1e-5 * xb.abs().max()
    assert (m0a - osch.outs[0].double()).abs().max() <= 1e-5 * m0a.abs().max()
    assert (xb - R.dpm_x_ref(xa, e2, None, z2, c2, dt=F64)).abs().max() > 1e-3            # the history term is really in it


_CASES = list(R.f16_floor_cases())
_KERNELS = ("groupnorm", "layernorm", "softmax_rows", "geglu", "gemv", "gemv_presum", "timestep_embed", "unpack_cfg", "adain_first", "adain_second", "dpm_step_x")


def test_every_f16_kernel_has_floor_cases():
    assert {c[0] for c in _CASES} == set(_KERNELS)
    assert len({(c[0], c[1]) for c in _CASES}) == len(_CASES)
    assert sum(c[0] == "groupnorm" for c in _CASES) == 2 * len(R.GN_CASES) and sum(c[0] == "layernorm" for c in _CASES) == len(R.LN_CASES)


@pytest.mark.parametrize("kernel", _KERNELS)
def test_f32_floor_within_cap(kernel):
    """floor = 4 x max|float32 - float64| of every case stays below ATOL_CAP (2e-3) of the output's RMS.  Largest floor per kernel: the docstring of
    tests/test_gpu_elem_leaves.py lists them."""
    worst, worst_frac = 0.0, 0.0
    for name, cid, fn, args in _CASES:
        if name != kernel:
            continue
        atol, rms = R.atol_of(name, cid)
        assert (atol, rms) == R.floor_atol(fn, *args)                       # what the GPU tests import is what is pinned here
        assert atol <= R.ATOL_CAP * rms, (name, cid, atol, rms)
        worst, worst_frac = max(worst, atol), max(worst_frac, atol / rms)
    print(f"[elem floor] {kernel}: largest floor {worst:.3e}, largest floor / RMS {worst_frac:.3e}")
