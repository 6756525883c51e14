"""GPU: leaf parity of the kernels either side of the UNet -- MemFlowNet / RAFT encoder and update-block glue, BriaRMBG, VAE layout kernels -- each through
the C ABI against a float64 evaluation of the same operation on the kernel's own rounded inputs (tests/leaf_refs.py, pinned by tests/test_leaf_refs_cpu.py).

Three classes of assertion (leaf_refs.py):
  exact       data movement and single-rounding kernels: torch.equal against the same IEEE sequence written in torch.
  f16 output  rel-L2 <= 2e-3 and, elementwise, |got - ref| <= 2^-10 |ref| + atol with atol = 4 x max|float32 - float64| of the same operation on the same
              inputs.  Largest atol per kernel: conv7x7s2_c3 8.0e-6, conv7x7s2_instnorm 1.2e-5, instnorm 2.0e-5, dwconv_gelu 8.8e-6, add_act (GELU) 3.5e-6,
              context_split (tanh) 1.3e-7, conv1x1_small 1.7e-6.
  f32 output  |got - ref| <= 3e-5 max(1, max|ref|).
Inputs are seeded, H != W; outputs and padding are prefilled with a sentinel wherever the kernel promises to leave or to zero them.  Every check prints
its figures (`-s`); profiles/producer_leaf_parity.txt keeps one run's."""
import pytest
import torch

import leaf_refs as R

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


def out32(*shape):
    return torch.full(shape, NAN, dtype=F32, device="cuda")


def ws_bytes(n):
    return torch.empty(int(n) + 256, dtype=torch.uint8, device="cuda")


def check_f16(name, case, got, ref, atol):
    """The two assertions of an f16-output kernel; got on the device, ref float64 on the CPU."""
    got = got.cpu()
    assert got.shape == ref.shape
    rel, ex = R.rel_l2(got, ref), R.elem_excess(got, ref, atol)
    print(f"[leaf] {name} {case}: rel-L2 {rel:.2e}  elementwise {ex:.3f} of (2^-10 |ref| + {atol:.2e})")
    assert not torch.isnan(got.float()).any(), (name, case)
    assert rel <= R.REL_F16, (name, case, rel)
    assert ex <= 1.0, (name, case, ex)


def check_f32(name, case, got, ref, magnitude=None):
    got = got.cpu().double()
    assert got.shape == ref.shape
    tol, err = R.f32_tol(ref, magnitude), (got - ref).abs().max().item()
    print(f"[leaf] {name} {case}: max|got - ref| {err:.2e}  (tolerance {tol:.2e})")
    assert not torch.isnan(got).any(), (name, case)
    assert err <= tol, (name, case, err, tol)


# ================================================================================================================== encoders
@pytest.mark.parametrize("Hh,Ww", R.STEM_SIZES)
def test_conv7x7s2_c3(L, Hh, Ww):
    """atol <= 8.0e-6 (513 output pixels: a ragged third block; 7x5: every window clipped)."""
    Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
    for relu in (0, 1):
        x, w, b = R.stem_input(Hh, Ww, Hh, False)
        y = out16(2, Ho, Wo, 64)
        L.tcl_conv7x7s2_c3_f16(dev(x), dev(R.stem_weight_t(w)), dev(b), y, 2, Hh, Ww, relu, st())
        check_f16("conv7x7s2_c3", (Hh, Ww, relu), y, R.conv7x7s2_ref(x, w, b, relu, dt=F64), R.atol_of("conv7x7s2_c3", (Hh, Ww, relu))[0])


@pytest.mark.parametrize("Hh,Ww", R.STEM_SIZES)
def test_conv7x7s2_instnorm(L, Hh, Ww):
    """Inputs in [0, 1] (a DC offset under the statistics); atol <= 1.2e-5."""
    Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
    x, w, b = R.stem_input(Hh, Ww, Hh + 1, True)
    y, ws = out16(2, Ho, Wo, 64), ws_bytes(L.tcl_stem_instnorm_workspace_bytes(2, Hh, Ww))
    L.tcl_conv7x7s2_instnorm_f16(dev(x), dev(R.stem_weight_t(w)), dev(b), y, 2, Hh, Ww, 1e-5, ws, st())
    check_f16("conv7x7s2_instnorm", (Hh, Ww), y, R.conv7x7s2_instnorm_ref(x, w, b, 1e-5, dt=F64), R.atol_of("conv7x7s2_instnorm", (Hh, Ww))[0])


@pytest.mark.parametrize("HW", R.INSTNORM_HW)
@pytest.mark.parametrize("C", R.INSTNORM_C)
def test_instnorm(L, C, HW):
    """Channel 1 all zero -> exactly 0; channel 2 mean 6 / std 0.05 within the same bound as the others; same bits on a reused workspace.  atol <= 2.0e-5."""
    for B in R.INSTNORM_B:
        x = R.instnorm_input(B, HW, C, C + HW + B)
        xd, ws = dev(x), ws_bytes(L.tcl_instnorm_workspace_bytes(B, C))
        atol = R.atol_of("instnorm", (C, HW, B))[0]
        for relu in (0, 1):
            y, y2 = out16(B, HW, C), out16(B, HW, C)
            L.tcl_instnorm_f16(xd, y, B, HW, C, 1e-5, relu, ws, st())
            L.tcl_instnorm_f16(xd, y2, B, HW, C, 1e-5, relu, ws, st())
            ref = R.instnorm_ref(x, 1e-5, relu, dt=F64)
            check_f16("instnorm", (C, HW, B, relu), y, ref, atol)
            check_f16("instnorm[mean 6, std 0.05]", (C, HW, B, relu), y[..., 2], ref[..., 2], atol)
            assert torch.equal(y[..., 1], torch.zeros_like(y[..., 1]))
            assert torch.equal(y.view(torch.int16), y2.view(torch.int16))


@pytest.mark.parametrize("n", [8, 8 * 1025 + 8])
def test_add_act_axpy(L, n):
    """act 0 / 3 and axpy are one f32 operation and one rounding: exact.  GELU (act 4): atol <= 3.5e-6; the first eight values are +-0, +-10, +-1e-3, +-3."""
    a, b = R.add_act_input(n, n)
    ad, bd = dev(a), dev(b)
    for act in (0, 3):
        y = out16(n)
        L.tcl_add_act_f16(ad, bd, y, n, act, st())
        t = a.float() + b.float()
        assert torch.equal(y.cpu(), (t.relu() if act else t).half()), act
    y = out16(n)
    L.tcl_add_act_f16(ad, bd, y, n, 4, st())
    check_f16("add_act_gelu", (n,), y, R.add_act_ref(a, b, 4, dt=F64), R.atol_of("add_act_gelu", (n,))[0])
    for s in (0.0, -1.5, 1.0):                 # s * f16 is exact in f32 for these: a fused multiply-add and mul + add round alike
        y = out16(n)
        L.tcl_axpy_f16(ad, bd, s, y, n, st())
        assert torch.equal(y.cpu(), (a.float() + s * b.float()).half()), s


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("Hh,Ww", [(5, 7), (4, 6), (1, 1)])
def test_subsample2(L, Hh, Ww, C):
    x = torch.randn(2, Hh, Ww, C, generator=R.rng(Hh + C)).half()
    y = out16(2, (Hh + 1) // 2, (Ww + 1) // 2, C)
    L.tcl_subsample2_nhwc_f16(dev(x), y, 2, Hh, Ww, C, st())
    assert torch.equal(y.cpu(), x[:, ::2, ::2].contiguous())


@pytest.mark.parametrize("D", [3, 64])
@pytest.mark.parametrize("Hh,Ww", [(5, 7), (2, 2), (9, 4)])
def test_avgpool2(L, Hh, Ww, D):
    x = torch.randn(2, Hh, Ww, D, generator=R.rng(Hh + D))
    y = out32(2, Hh // 2, Ww // 2, D)
    L.tcl_avgpool2_nhwc_f32(dev(x), y, 2, Hh, Ww, D, st())
    check_f32("avgpool2_nhwc", (Hh, Ww, D), y, R.avgpool2_nhwc_ref(x, dt=F64))


# ================================================================================================================== update block
@pytest.mark.parametrize("P", [1, 257])
def test_context_split(L, P):
    """relu half exact; tanh half atol <= 1.3e-7, values to +-9."""
    c = R.context_input(P, P)
    net, inp = out16(P, 128), out16(P, 128)
    L.tcl_context_split_f16(dev(c), net, inp, P, st())
    assert torch.equal(inp.cpu(), c[:, 128:].float().relu().half())
    check_f16("context_split_tanh", (P,), net, R.tanh_ref(c[:, :128], dt=F64), R.atol_of("context_split_tanh", (P,))[0])


@pytest.mark.parametrize("Hh,Ww", R.DW_SIZES)
@pytest.mark.parametrize("C", R.DW_C)
@pytest.mark.parametrize("k", R.DW_K)
def test_dwconv_gelu(L, k, C, Hh, Ww):
    """5x3: all halo; 16x16: one tile; 17x33: tile tails on both axes; atol <= 8.8e-6."""
    x, w, b = R.dwconv_input(k, C, Hh, Ww, k + C + Hh)
    y = out16(2, Hh, Ww, C)
    L.tcl_dwconv_gelu_f16(dev(x), dev(w), dev(b), y, 2, Hh, Ww, C, k, st())
    check_f16("dwconv_gelu", (k, C, Hh, Ww), y, R.dwconv_gelu_ref(x, w, b, k, dt=F64), R.atol_of("dwconv_gelu", (k, C, Hh, Ww))[0])


@pytest.mark.parametrize("Cs,ld,c0", [(2, 16, 0), (2, 16, 5), (81, 96, 8)])
def test_nchw_rows_roundtrip(L, Cs, ld, c0):
    B, P = 2, 77
    x = torch.randn(B, Cs, P, generator=R.rng(Cs + c0)) * 3
    want = x.half().permute(0, 2, 1).reshape(B * P, Cs)
    for zero_rest in (0, 1):
        rows = out16(B * P, ld)
        L.tcl_nchw_f32_to_rows_f16(dev(x), rows, B, Cs, P, ld, c0, zero_rest, st())
        r = rows.cpu()
        assert torch.equal(r[:, c0:c0 + Cs], want)
        rest = torch.cat([r[:, :c0], r[:, c0 + Cs:]], 1)
        assert torch.equal(rest, torch.zeros_like(rest)) if zero_rest else R.is_sentinel16(rest)
    # the reverse: alpha = 0 overwrites (no NaN of the output may survive) and is exact; then out = alpha*out + beta*value
    src = R.sentinel16(B * P, ld)
    src[:, c0:c0 + Cs] = want
    srcd, back = dev(src), out32(B, Cs, P)
    L.tcl_rows_f16_to_nchw_f32(srcd, back, B, Cs, P, ld, c0, 0.0, 1.0, st())
    assert torch.equal(back.cpu(), x.half().float())
    y0 = torch.randn(B, Cs, P, generator=R.rng(9))
    for alpha, beta in ((1.0, 1.0), (0.5, -2.0)):
        y = dev(y0)
        L.tcl_rows_f16_to_nchw_f32(srcd, y, B, Cs, P, ld, c0, alpha, beta, st())
        check_f32("rows_f16_to_nchw_f32", (Cs, ld, c0, alpha, beta), y, alpha * y0.double() + beta * x.half().double())


@pytest.mark.parametrize("ldm", [576, 640])
@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (2, 3, 5), (1, 12, 20)])
def test_upsample_flow(L, B, h, w, ldm):
    """Flows to +-20 (tolerance on max|8 flow|); ldm 640 carries NaN in columns 576..639; the last pass has logits of +-3e4 (max-subtraction)."""
    g = R.rng(B + h + ldm)
    flow = (torch.rand(B, 2, h, w, generator=g) * 40 - 20)
    flow[0, 0, 0, 0], flow[0, 1, -1, -1] = 20.0, -20.0
    for big in (False, True):
        m = (torch.randn(B * h * w, 576, generator=g) * 4).half()
        if big:
            m = torch.where(torch.rand(B * h * w, 576, generator=g) < 0.5, torch.tensor(3e4), torch.tensor(-3e4)).half()
        rows = torch.full((B * h * w, ldm), NAN, dtype=H)
        rows[:, :576] = m
        for scale in (0.25, 1.0):
            up = out32(B, 2, 8 * h, 8 * w)
            L.tcl_upsample_flow_f32(dev(flow), dev(rows), ldm, scale, up, B, h, w, st())
            check_f32("upsample_flow", (B, h, w, ldm, scale, "3e4" if big else ""), up, R.upsample_flow_ref(flow, rows, scale, dt=F64),
                      magnitude=(8 * flow).abs().max())


# ================================================================================================================== BriaRMBG
@pytest.mark.parametrize("C1,C2,Cout,dil,stride,relu,resid,Hh,Ww", R.CONV3X3)
def test_conv3x3_direct(L, C1, C2, Cout, dil, stride, relu, resid, Hh, Ww):
    g = R.rng(C1 + Cout + dil)
    B, Cin = 2, C1 + C2
    x1 = torch.randn(B, C1, Hh, Ww, generator=g)
    x2 = torch.randn(B, C2, Hh, Ww, generator=g) if C2 else None
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    scale, shift = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g) * 0.5
    scale[0] = -abs(scale[0]) - 0.1
    Ho, Wo = (Hh - 1) // stride + 1, (Ww - 1) // stride + 1
    r = torch.randn(B, Cout, Ho, Wo, generator=g) if resid else None
    y = out32(B, Cout, Ho, Wo)
    L.tcl_conv3x3_direct_f32(dev(x1), C1, dev(x2) if C2 else 0, C2, dev(R.conv3x3_weight_t(w)), dev(scale), dev(shift), dev(r) if resid else 0, y,
                             B, Hh, Ww, Cout, dil, stride, relu, st())
    check_f32("conv3x3_direct", (C1, C2, Cout, dil, stride, Hh, Ww), y, R.conv3x3_direct_ref(x1, x2, w, scale, shift, r, dil, stride, relu, dt=F64))


@pytest.mark.parametrize("Hh,Ww", [(5, 7), (4, 6), (1, 1), (1, 9)])
def test_maxpool2_ceil(L, Hh, Ww):
    """All-negative inputs: padding the ragged row / column with 0 instead of -inf would win the maximum."""
    x = -torch.rand(6, Hh, Ww, generator=R.rng(Hh + Ww)) - 0.25
    y = out32(6, (Hh + 1) // 2, (Ww + 1) // 2)
    L.tcl_maxpool2_ceil_f32(dev(x), y, 6, Hh, Ww, st())
    assert torch.equal(y.cpu(), R.maxpool2_ceil_ref(x[None], dt=F32)[0])


@pytest.mark.parametrize("Hh,Ww,Ho,Wo", R.RESIZE)
def test_resize_bilinear(L, Hh, Ww, Ho, Wo):
    x = torch.randn(3, Hh, Ww, generator=R.rng(Hh + Ho))
    xd = dev(x)
    for mul in (1.0, 0.5):
        for sig, cl in ((0, 0), (1, 0), (0, 1), (1, 1)):
            y = out32(3, Ho, Wo)
            L.tcl_resize_bilinear_f32(xd, y, 3, Hh, Ww, Ho, Wo, mul, sig, cl, st())
            check_f32("resize_bilinear", (Hh, Ww, Ho, Wo, mul, sig, cl), y, R.resize_bilinear_ref(x[None], Ho, Wo, mul, sig, cl, dt=F64)[0])


def test_resize_bilinear_identity(L):
    x = torch.randn(3, 6, 6, generator=R.rng(66)) * 2
    y = out32(3, 6, 6)
    L.tcl_resize_bilinear_f32(dev(x), y, 3, 6, 6, 6, 6, 1.0, 0, 0, st())
    assert torch.equal(y.cpu(), x)


# ================================================================================================================== VAE glue
def test_img_nhwc8(L):
    B, HW = 2, 5 * 7
    img = torch.rand(B, 3, HW, generator=R.rng(1))
    out = out16(B, HW, 8)
    L.tcl_img_to_nhwc8_f16(dev(img), out, B, HW, st())
    o = out.cpu()
    assert torch.equal(o[..., :3], (2.0 * img - 1.0).half().permute(0, 2, 1)) and torch.equal(o[..., 3:], torch.zeros(B, HW, 5).half())


@pytest.mark.parametrize("ldc", [8, 128])
def test_nhwc_to_img(L, ldc):
    B, HW = 2, 5 * 7
    y = R.sentinel16(B, HW, ldc)
    y[..., :3] = (torch.randn(B, HW, 3, generator=R.rng(ldc)) * 1.5).half()          # values outside [-1, 1] on both sides
    assert y[..., :3].float().max() > 1 and y[..., :3].float().min() < -1
    img = out32(B, 3, HW)
    L.tcl_nhwc_to_img_f32(dev(y), ldc, img, B, HW, st())
    assert torch.equal(img.cpu(), (y[..., :3].float() * 0.5 + 0.5).half().float().clamp(0, 1).permute(0, 2, 1))


@pytest.mark.parametrize("scale", [0.18215, 1 / 0.18215])
@pytest.mark.parametrize("ldc", [8, 64])
def test_nhwc_nchw(L, ldc, scale):
    B, C, HW = 2, 4, 5 * 7
    y = R.sentinel16(B, HW, ldc)
    y[..., :C] = torch.randn(B, HW, C, generator=R.rng(ldc)).half()
    z = out16(B, C, HW)
    L.tcl_nhwc_to_nchw_f16(dev(y), ldc, z, B, C, HW, scale, st())
    s32 = torch.tensor(scale, dtype=F32)
    assert torch.equal(z.cpu(), (y[..., :C].float() * s32).half().permute(0, 2, 1))
    x = torch.randn(B, C, HW, generator=R.rng(ldc + 1)).half()
    back = out16(B, HW, ldc)
    L.tcl_nchw_to_nhwc_f16(dev(x), back, ldc, B, C, HW, scale, st())
    b = back.cpu()
    assert torch.equal(b[..., :C], (x.float() * s32).half().permute(0, 2, 1)) and torch.equal(b[..., C:], torch.zeros(B, HW, ldc - C).half())


@pytest.mark.parametrize("Rr,Cc", [(33, 65), (1, 40)])
def test_transpose(L, Rr, Cc):
    batch, ldi, ldo = 2, Cc + 7, Rr + 3
    a = R.sentinel16(batch, Rr, ldi)
    a[..., :Cc] = torch.randn(batch, Rr, Cc, generator=R.rng(Rr)).half()
    out = out16(batch, Cc, ldo)
    L.tcl_transpose_f16(dev(a), out, batch, Rr, Cc, ldi, ldo, st())
    o = out.cpu()
    assert torch.equal(o[..., :Rr], a[..., :Cc].transpose(1, 2)) and R.is_sentinel16(o[..., Rr:])


@pytest.mark.parametrize("M", [1, 1000])
@pytest.mark.parametrize("Ci,Co,ldi,ldo", R.CONV1X1)
def test_conv1x1_small(L, Ci, Co, ldi, ldo, M):
    """Columns Ci.. of the input rows hold the sentinel (never read), columns Co..ldo of the output come out zero; atol <= 1.7e-6."""
    x, W, b = R.conv1x1_input(Ci, Co, M, Ci + Co + ldi + M)
    xs = R.sentinel16(M, ldi)
    xs[:, :Ci] = x
    y = out16(M, ldo)
    L.tcl_conv1x1_small_f16(dev(xs), ldi, dev(W), dev(b), y, ldo, M, Ci, Co, st())
    check_f16("conv1x1_small", (Ci, Co, ldi, ldo, M), y[:, :Co], R.conv1x1_small_ref(x, W, b, dt=F64), R.atol_of("conv1x1_small", (Ci, Co, ldi, ldo, M))[0])
    assert torch.equal(y[:, Co:].cpu(), torch.zeros(M, ldo - Co).half())


@pytest.mark.parametrize("Hh,Ww", [(1, 1), (3, 5), (9, 13)])
@pytest.mark.parametrize("Cin,Kpad", [(3, 64), (4, 64), (8, 128), (3, 128)])
def test_im2col3x3_small(L, Cin, Kpad, Hh, Ww):
    x = torch.randn(2, Hh, Ww, Cin, generator=R.rng(Cin + Hh)).half()
    out = out16(2 * Hh * Ww, Kpad)
    L.tcl_im2col3x3_small_f16(dev(x), out, 2, Hh, Ww, Cin, Kpad, st())
    assert torch.equal(out.cpu(), R.im2col3x3_ref(x, Kpad))


@pytest.mark.parametrize("rows", [1, 1001])
def test_concat_channels(L, rows):
    g = R.rng(rows)
    a, b = torch.randn(rows, 8, generator=g).half(), torch.randn(rows, 24, generator=g).half()
    y = out16(rows, 32)
    L.tcl_concat_channels_f16(dev(a), 8, dev(b), 24, y, rows, st())
    assert torch.equal(y.cpu(), torch.cat([a, b], 1))


# ================================================================================================================== refused arguments
def test_refused_arguments(L):
    """Every entry returns TCL_EINVAL before any launch: nothing runs on the device."""
    h, f, ws = out16(4096), out32(4096), ws_bytes(1 << 20)
    bad = [
        lambda: L.tcl_instnorm_f16(h, h, 1, 4, 40, 1e-5, 0, ws, st()),
        lambda: L.tcl_instnorm_f16(h, h, 1, 4, 264, 1e-5, 0, ws, st()),
        lambda: L.tcl_add_act_f16(h, h, h, 12, 0, st()),
        lambda: L.tcl_add_act_f16(h, h, h, 8, 1, st()),
        lambda: L.tcl_dwconv_gelu_f16(h, h, h, h, 1, 4, 4, 8, 3, st()),
        lambda: L.tcl_upsample_flow_f32(f, h, 512, 0.25, f, 1, 1, 1, st()),
        lambda: L.tcl_avgpool2_nhwc_f32(f, f, 1, 1, 4, 64, st()),
        lambda: L.tcl_conv1x1_small_f16(h, 16, h, h, h, 16, 4, 9, 8, st()),
        lambda: L.tcl_im2col3x3_small_f16(h, h, 1, 2, 2, 4, 100, st()),
        # the layout kernels: empty batches and strides narrower than the channels they carry
        lambda: L.tcl_img_to_nhwc8_f16(f, h, 0, 4, st()),
        lambda: L.tcl_nhwc_to_img_f32(h, 8, f, 0, 4, st()),
        lambda: L.tcl_nhwc_to_img_f32(h, 2, f, 1, 4, st()),
        lambda: L.tcl_nhwc_to_nchw_f16(h, 8, h, 0, 4, 4, 1.0, st()),
        lambda: L.tcl_nhwc_to_nchw_f16(h, 2, h, 1, 4, 4, 1.0, st()),
        lambda: L.tcl_nchw_to_nhwc_f16(h, h, 8, -1, 4, 4, 1.0, st()),
        lambda: L.tcl_nchw_to_nhwc_f16(h, h, 2, 1, 4, 4, 1.0, st()),
        lambda: L.tcl_transpose_f16(h, h, 0, 4, 4, 4, 4, st()),
        lambda: L.tcl_transpose_f16(h, h, 1, 4, 8, 4, 4, st()),
        lambda: L.tcl_conv1x1_small_f16(h, 4, h, h, h, 8, 4, 8, 8, st()),
        lambda: L.tcl_concat_channels_f16(h, 8, h, 24, h, 0, st()),
        lambda: L.tcl_im2col3x3_small_f16(h, h, 0, 2, 2, 4, 64, st()),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            call()
    torch.cuda.synchronize()
    assert R.is_sentinel16(h.cpu()) and torch.isnan(f).all()
