"""GPU: leaf parity of the kernels of csrc/elem.hip that run between the GEMMs of the UNet, in the VAE and in every sampler step -- GroupNorm (+ SiLU,
concat, yraw), LayerNorm (+ metric), row softmax (register and LDS form), GEGLU, GEMV, timestep embedding, CFG unpack, AdaIN fusion, the SDE-DPM-Solver++
update -- each through the C ABI against a float64 evaluation of the same operation on the kernel's own rounded inputs (tests/elem_refs.py, pinned by
tests/test_elem_refs_cpu.py).

Classes of assertion (elem_refs.py):
  exact       torch.equal: yraw, y with and without yraw, a sample alone against the same sample in a batch, a second call on the same workspace, the
              LayerNorm metric against tcl_tome_normalize_f16, LayerNorm of a constant row, every byte a kernel promises to leave alone (f16 sentinel).
  f16 output  rel-L2 <= 2e-3 and, elementwise, |got - ref| <= 2^-10 |ref| + atol, atol = 4 x max|float32 - float64| of the same operation on the same
              inputs + 2^-24.  GroupNorm takes the elementwise maximum per (sample, group) and prints the worst group.  Largest atol per kernel in the recorded
              run: groupnorm 6.7e-5 (3.2e-4 with offset 4, 7.2e-4 with gamma x 64), layernorm 8.2e-6, softmax_rows 3.9e-6 (register form) / 1.0e-6
              (LDS form), geglu 1.3e-5, gemv 1.2e-4, timestep_embed 2.1e-4, unpack_cfg 5.3e-7, adain 2.1e-6 / 1.7e-6, dpm_step x 2.0e-6.
  f32 output  m0 of the DPM step: |got - ref| <= 2^-22 max(1, |ref|) elementwise.
Inputs are seeded; outputs and padding are prefilled with the f16 sentinel (NaN for f32) and workspaces with 0xFF bytes.  Every check prints its figures
(`-s`); profiles/elem_leaf_parity.txt keeps one run's."""
import pytest
import torch

import elem_refs as R

pytestmark = pytest.mark.gpu
H, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float("nan")


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


def out16(*shape):
    return dev(R.sentinel16(*shape))


def bits(t):
    return t.contiguous().view(torch.int16)


def check_f16(name, case, got, ref, floor):
    """The two assertions of an f16-output kernel; got f16 (device or host), ref float64 on the CPU; atol = floor + 2^-24."""
    got, atol = got.cpu(), floor + R.SUB16
    assert got.shape == ref.shape
    rel, ex = R.rel_l2(got, ref), R.elem_excess(got, ref, atol)
    print(f"[elem] {name} {case}: rel-L2 {rel:.2e}  elementwise {ex:.3f} of (2^-10 |ref| + {atol:.2e})")
    assert not torch.isnan(got.float()).any(), (name, case)
    assert rel <= R.REL_F16, (name, case, rel)
    assert ex <= 1.0, (name, case, ex)


# ================================================================================================================== GroupNorm
def _groupnorm(L, x1, x2, ga, be, y, yraw, G, silu, ws):
    B, HW, C1 = x1.shape
    C2 = x2.shape[2] if x2 is not None else 0
    if yraw is None:
        L.tcl_groupnorm_f16(x1, C1, x2 if C2 else 0, C2, ga, be, y, B, HW, G, R.EPS_GN, silu, ws, st())
    else:
        L.tcl_groupnorm_concat_f16(x1, C1, x2 if C2 else 0, C2, ga, be, y, yraw, B, HW, G, R.EPS_GN, silu, ws, st())


def _ws(L, B, C):
    return torch.full((int(L.tcl_groupnorm_workspace_bytes(B, C)),), 0xFF, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("shape,kind,gscale", R.GN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_groupnorm(L, shape, kind, gscale):
    """Elementwise bound per (sample, group) against the two-pass float64 GroupNorm; yraw == the concat; y the same bits with and without yraw, on a
    reused workspace, and for every sample alone (the contract above gn_blocks_cap in csrc/elem.hip)."""
    B, HW, C1, C2, G = shape
    C = C1 + C2
    x1, x2, ga, be = R.gn_input(shape, kind, gscale)
    d1, d2, dga, dbe = dev(x1), (dev(x2) if C2 else None), dev(ga), dev(be)
    ws = _ws(L, B, C)
    for silu in (0, 1):
        floor = R.atol_of("groupnorm", (shape, kind, gscale, silu))[0]
        atol = floor + R.SUB16
        y, yraw, y2, y3 = out16(B, HW, C), out16(B, HW, C), out16(B, HW, C), out16(B, HW, C)
        _groupnorm(L, d1, d2, dga, dbe, y, yraw, G, silu, ws)
        _groupnorm(L, d1, d2, dga, dbe, y2, yraw, G, silu, ws)                 # the same workspace again
        _groupnorm(L, d1, d2, dga, dbe, y3, None, G, silu, ws)                 # tcl_groupnorm_f16: the null-yraw kernels
        got = y.cpu()
        ref = R.groupnorm_two_pass_ref(x1, x2, ga, be, G, R.EPS_GN, silu)
        q = R.group_excess(got, ref, atol, G)
        wb, wg = divmod(int(q.argmax()), G)
        rel = R.rel_l2(got, ref)
        print(f"[elem] groupnorm {shape} {kind} gamma x{gscale} silu {silu}: rel-L2 {rel:.2e}  worst group (sample {wb}, group {wg}) {q.max().item():.3f} "
              f"of (2^-10 |ref| + {atol:.2e})")
        assert not torch.isnan(got.float()).any()
        assert rel <= R.REL_F16, rel
        assert (q <= 1.0).all(), [(b, g, round(q[b, g].item(), 2)) for b, g in (q > 1.0).nonzero().tolist()][:8]
        assert torch.equal(bits(yraw.cpu()), bits(x1 if x2 is None else torch.cat([x1, x2], -1)))
        assert torch.equal(bits(y2), bits(y)), "second call on the same workspace"
        assert torch.equal(bits(y3), bits(y)), "with and without yraw"
        if B > 1:
            for b in range(B):
                ys, ws1 = out16(1, HW, C), _ws(L, 1, C)
                _groupnorm(L, d1[b:b + 1].contiguous(), d2[b:b + 1].contiguous() if C2 else None, dga, dbe, ys, None, G, silu, ws1)
                assert torch.equal(bits(ys[0]), bits(y[b])), f"sample {b} alone"


def test_groupnorm_refuses_three_groups_per_chunk(L):
    """cpg = 5 (C = 160, G = 32): the 8-channel chunk at channel 8 holds groups 1, 2 and 3; the kernels split a chunk once.  TCL_EINVAL, as the wrapper
    reports it, before any launch: both outputs keep the sentinel."""
    B, HW, C1, C2, G = R.GN_REFUSED
    g = R.rng(5)
    x, ga, be = dev((torch.randn(B, HW, C1, generator=g) * 2 + 0.5).to(H)), dev(torch.randn(C1, generator=g).to(H)), dev(torch.randn(C1, generator=g).to(H))
    y, yraw, ws = out16(B, HW, C1), out16(B, HW, C1), _ws(L, B, C1)
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_groupnorm_concat_f16(x, C1, 0, 0, ga, be, y, yraw, B, HW, G, R.EPS_GN, 1, ws, st())
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_groupnorm_f16(x, C1, 0, 0, ga, be, y, B, HW, G, R.EPS_GN, 0, ws, st())
    torch.cuda.synchronize()
    assert R.is_sentinel16(y.cpu()) and R.is_sentinel16(yraw.cpu()) and bool((ws == 0xFF).all())


# ================================================================================================================== LayerNorm
@pytest.mark.parametrize("C", R.LN_C)
def test_layernorm(L, C):
    """y in the f16 class; the metric entry gives the same y bits and the bits of tcl_tome_normalize_f16(y); rows past `rows` keep the sentinel; a constant
    row comes out as beta exactly."""
    for Cc, rows, kind in R.LN_CASES:
        if Cc != C:
            continue
        x, ga, be = R.ln_input(C, rows, kind)
        dx, dga, dbe = dev(x), dev(ga), dev(be)
        pad = 5
        y, y2, m2, m = (out16(rows + pad, C) for _ in range(4))
        L.tcl_layernorm_f16(dx, dga, dbe, y, rows, C, R.EPS_LN, st())
        L.tcl_layernorm_metric_f16(dx, dga, dbe, y2, m2, rows, C, R.EPS_LN, st())
        L.tcl_tome_normalize_f16(y, m, rows, C, st())
        got = y.cpu()
        check_f16("layernorm", (C, rows, kind), got[:rows], R.layernorm_ref(x, ga, be, R.EPS_LN, dt=F64), R.atol_of("layernorm", (C, rows, kind))[0])
        assert torch.equal(bits(y2), bits(y)) and torch.equal(bits(m2), bits(m)), (C, rows, kind)
        assert R.is_sentinel16(got[rows:]) and R.is_sentinel16(m2[rows:].cpu())
        if kind == "const":
            assert torch.equal(got[R.LN_CONST_ROW], be)


# ================================================================================================================== row softmax
@pytest.mark.parametrize("T,ld,form", R.SOFTMAX_CASES)
def test_softmax_rows(L, T, ld, form):
    """In place on [3, ld] with columns T.. holding the sentinel; f16 class, row sums within T 2^-11 of 1, the argmax preserved."""
    assert R.softmax_form(T, ld) == form
    for kind in R.softmax_kinds(T):
        x = R.softmax_input(T, kind)
        buf = R.sentinel16(R.SOFTMAX_ROWS, ld)
        buf[:, :T] = x
        d = dev(buf)
        L.tcl_softmax_rows_f16(d, R.SOFTMAX_ROWS, T, ld, R.SOFTMAX_SCALE, st())
        got = d.cpu()
        ref = R.softmax_ref(x, R.SOFTMAX_SCALE, dt=F64)
        check_f16(f"softmax_rows[{form}]", (T, ld, kind), got[:, :T], ref, R.atol_of("softmax_rows", (T, ld, kind))[0])
        assert R.is_sentinel16(got[:, T:])
        sums = got[:, :T].double().sum(1)
        print(f"[elem] softmax_rows[{form}] {(T, ld, kind)}: max |row sum - 1| {(sums - 1).abs().max().item():.2e}  (bound {T * 2.0 ** -11:.2e})")
        assert ((sums - 1).abs() <= T * 2.0 ** -11).all()
        am = ref.argmax(1, keepdim=True)
        assert torch.equal(got[:, :T].float().gather(1, am)[:, 0], got[:, :T].float().amax(1))


# ================================================================================================================== GEGLU / GEMV / timestep embedding
@pytest.mark.parametrize("D,rows", R.GEGLU_CASES)
def test_geglu(L, D, rows):
    x = R.geglu_input(D, rows)
    y = out16(rows + 1, D)
    L.tcl_geglu_f16(dev(x), y, rows, D, st())
    check_f16("geglu", (D, rows), y[:rows], R.geglu_ref(x, dt=F64), R.atol_of("geglu", (D, rows))[0])
    assert R.is_sentinel16(y[rows:].cpu())


@pytest.mark.parametrize("N,K", R.GEMV_SHAPES)
def test_gemv(L, N, K):
    """The reference rounds SiLU(x) to f16 before the product and the sum to f16 before `add`, as the kernel does.  A sum within its float32 floor of an f16
    rounding tie may round to either neighbour in the kernel: such an output is held to the nearer of the two references (their number is printed)."""
    for fl in R.GEMV_FLAGS:
        silu_in, silu_out, has_b, has_a = fl
        W, x, b, a = R.gemv_input(N, K, fl)
        y = out16(N + 3)
        L.tcl_gemv_f16(dev(W), dev(x), dev(b) if has_b else 0, dev(a) if has_a else 0, y, N, K, silu_in, silu_out, st())
        got = y.cpu()
        assert R.is_sentinel16(got[N:])
        ref = R.gemv_ref(W, x, b if has_b else None, a if has_a else None, silu_in, silu_out, dt=F64)
        floor = R.atol_of("gemv", (N, K, fl))[0]
        if has_a:
            amb, alt = R.gemv_alt_ref(W, x, b if has_b else None, a, silu_in, silu_out, R.atol_of("gemv_presum", (N, K, fl))[0])
            take = amb & ((got[:N].double() - alt).abs() < (got[:N].double() - ref).abs())
            print(f"[elem] gemv {(N, K, fl)}: {int(amb.sum())} of {N} sums within the float32 floor of an f16 rounding tie, {int(take.sum())} rounded the other way")
            ref = torch.where(take, alt, ref)
        check_f16("gemv", (N, K, fl), got[:N], ref, floor)


@pytest.mark.parametrize("t", R.TEMB_T)
def test_timestep_embed(L, t):
    y = out16(R.TEMB_DIM + 8)
    L.tcl_timestep_embed_f16(t, R.TEMB_DIM, y, st())
    check_f16("timestep_embed", (t,), y[:R.TEMB_DIM], R.timestep_embed_ref(t, R.TEMB_DIM, dt=F64), R.atol_of("timestep_embed", (t,))[0])
    assert R.is_sentinel16(y[R.TEMB_DIM:].cpu())


# ================================================================================================================== sampler glue
@pytest.mark.parametrize("case", R.UNPACK_CASES, ids=lambda c: c[0])
def test_unpack_cfg(L, case):
    """xy: frames outside idx keep the sentinel.  yt with nkeep < nwin: frames sl + nkeep .. and every column outside the list keep it."""
    name, mode, idx, sl, nwin, guidance, scale_upto, scale, nkeep = case
    eps = R.unpack_input(case)
    noise = out16(R.UNPACK_N, 4, R.UNPACK_H, R.UNPACK_W)
    L.tcl_unpack_cfg_f16(dev(eps), dev(torch.tensor(idx, dtype=torch.int32)), len(idx), mode, sl, nwin, R.UNPACK_H, R.UNPACK_W, guidance, scale_upto, scale,
                         nkeep, noise, st())
    got = noise.cpu()
    ref, mask = R.unpack_cfg_ref(eps, case, dt=F64)
    assert mask.any() and not mask.all()
    check_f16("unpack_cfg", (name,), got[mask], ref[mask], R.atol_of("unpack_cfg", (name,))[0])
    assert R.is_sentinel16(got[~mask])


@pytest.mark.parametrize("hw", R.ADAIN_HW)
def test_adain_fuse(L, hw):
    """Both outputs; the second against the formula applied to the kernel's own ROUNDED first output."""
    a, b = R.adain_input(hw)
    buf_a, buf_b = R.sentinel16(R.ADAIN_PLANES + 1, hw), R.sentinel16(R.ADAIN_PLANES + 1, hw)
    buf_a[:-1], buf_b[:-1] = a, b
    da, db = dev(buf_a), dev(buf_b)
    L.tcl_adain_fuse_f16(da, db, R.ADAIN_PLANES, hw, R.ADAIN_ALPHA, st())
    ga, gb = da.cpu(), db.cpu()
    check_f16("adain_first", (hw,), ga[:-1], R.adain_first_ref(a, b, dt=F64), R.atol_of("adain_first", (hw,))[0])
    check_f16("adain_second", (hw,), gb[:-1], R.adain_second_ref(ga[:-1], b, R.ADAIN_ALPHA, dt=F64), R.atol_of("adain_second", (hw,))[0])
    assert R.is_sentinel16(ga[-1]) and R.is_sentinel16(gb[-1])


@pytest.mark.parametrize("n,second,with_z", R.DPM_CASES)
def test_dpm_sde_step(L, n, second, with_z):
    """Coefficients of tc_light_amd.scheduler for the first two executed steps of the 20-step schedule entered at index 15.  x f16 class, m0 f32 class;
    m1 and eps unchanged; nothing written past n."""
    coef = R.dpm_coefficients(second)
    x, eps, m1, z = R.dpm_input(n, second, with_z)
    xb = R.sentinel16(n + 8)
    xb[:n] = x
    dx, de = dev(xb), dev(eps)
    m0 = torch.full((n + 8,), NAN, dtype=F32, device="cuda")
    dm1, dz = (dev(m1) if second else None), (dev(z) if with_z else None)
    L.tcl_dpm_sde_step_f16(dx, de, m0, dm1 if second else 0, dz if with_z else 0, n, *coef, st())
    gx, gm = dx.cpu(), m0.cpu()
    check_f16("dpm_step_x", (n, second, with_z), gx[:n], R.dpm_x_ref(x, eps, m1, z, coef, dt=F64), R.atol_of("dpm_step_x", (n, second, with_z))[0])
    ref0 = R.dpm_m0_ref(x, eps, coef, dt=F64)
    q = ((gm[:n].double() - ref0).abs() / (R.F32_REL * ref0.abs().clamp_min(1.0))).max().item()
    print(f"[elem] dpm_step_m0 {(n, second, with_z)}: elementwise {q:.3f} of 2^-22 max(1, |ref|)")
    assert q <= 1.0, q
    assert R.is_sentinel16(gx[n:]) and torch.isnan(gm[n:]).all()
    assert torch.equal(de.cpu(), eps) and (not second or torch.equal(dm1.cpu(), m1)) and (not with_z or torch.equal(dz.cpu(), z))
