"""CPU: the float64 references of tests/leaf_refs.py against oracle/ (itself pinned to goldens of the reference), and the float32-against-float64
floors the GPU leaf tests take their elementwise atol from.  A wrong reference or a loose floor then cannot pass quietly."""
import pytest
import torch
import torch.nn.functional as F

import leaf_refs as R
from oracle import memflow as OM
from oracle import rmbg as OR

F64 = torch.float64


def close12(a, b):
    return (a - b).abs().max().item() <= 1e-12


def test_dwconv_ref_vs_oracle_pcblock():
    """oracle.memflow.pcblock with its depthwise stages replaced by dwconv_gelu_ref (NHWC, tap-major [k*k, C] weights): same block to 1e-12."""
    g, C = R.rng(1), 8
    sd = {}
    for q in ("ffn1.", "ffn2."):
        for i, (co, ci) in ((0, (12, C)), (2, (C, 12))):
            sd[f"p.{q}{i}.weight"], sd[f"p.{q}{i}.bias"] = torch.randn(co, ci, 1, 1, generator=g, dtype=F64) / 3, torch.randn(co, generator=g, dtype=F64) / 3
    sd["p.pw.weight"], sd["p.pw.bias"] = torch.randn(C, C, 1, 1, generator=g, dtype=F64) / 3, torch.randn(C, generator=g, dtype=F64) / 3
    ks = (1, 7, 15)
    taps = [torch.randn(k * k, C, generator=g, dtype=F64) / k for k in ks]
    for i, k in enumerate(ks):
        sd[f"p.conv_list.{i}.weight"], sd[f"p.conv_list.{i}.bias"] = R.dw_weight_conv(taps[i], k).contiguous(), torch.randn(C, generator=g, dtype=F64) / 3
    x = torch.randn(2, C, 9, 13, generator=g, dtype=F64)
    want = OM.pcblock(sd, "p.", x, ks)

    def ffn(q, t):
        return F.conv2d(F.gelu(F.conv2d(t, sd[q + "0.weight"], sd[q + "0.bias"])), sd[q + "2.weight"], sd[q + "2.bias"])
    y = F.gelu(x + ffn("p.ffn1.", x)).permute(0, 2, 3, 1)
    for i, k in enumerate(ks):
        y = R.dwconv_gelu_ref(y, taps[i], sd[f"p.conv_list.{i}.bias"], k, dt=F64)
    y = y.permute(0, 3, 1, 2)
    got = ffn("p.ffn2.", F.gelu(y + F.conv2d(y, sd["p.pw.weight"], sd["p.pw.bias"])))
    assert close12(got, want)
    # a ky/kx swap of the tap order must be visible: the seeded weights are not isotropic
    assert not close12(R.dwconv_gelu_ref(x.permute(0, 2, 3, 1), taps[1].view(7, 7, C).transpose(0, 1).reshape(49, C), sd["p.conv_list.1.bias"], 7, dt=F64),
                       R.dwconv_gelu_ref(x.permute(0, 2, 3, 1), taps[1], sd["p.conv_list.1.bias"], 7, dt=F64))


def test_upsample_flow_ref_vs_oracle():
    g = R.rng(2)
    B, h, w = 2, 3, 5
    flow = torch.randn(B, 2, h, w, generator=g, dtype=F64) * 10
    m = torch.randn(B, 576, h, w, generator=g, dtype=F64) * 4
    rows = torch.full((B * h * w, 640), float("nan"), dtype=F64)
    rows[:, :576] = m.permute(0, 2, 3, 1).reshape(-1, 576)
    assert close12(R.upsample_flow_ref(flow, rows, 0.25, dt=F64), OM.upsample_flow(flow, 0.25 * m))


@pytest.mark.parametrize("dil", [1, 2, 8])
def test_conv3x3_direct_ref_vs_oracle_rebnconv(dil):
    g = R.rng(3 + dil)
    Cin, Cout = 6, 5
    sd = {"c.conv_s1.weight": torch.randn(Cout, Cin, 3, 3, generator=g, dtype=F64) / 7, "c.conv_s1.bias": torch.randn(Cout, generator=g, dtype=F64),
          "c.bn_s1.running_mean": torch.randn(Cout, generator=g, dtype=F64), "c.bn_s1.running_var": torch.rand(Cout, generator=g, dtype=F64) + 0.5,
          "c.bn_s1.weight": torch.randn(Cout, generator=g, dtype=F64), "c.bn_s1.bias": torch.randn(Cout, generator=g, dtype=F64)}
    sd["c.bn_s1.weight"][0] = -0.75                      # negative scales are part of the contract
    x = torch.randn(2, Cin, 5, 7, generator=g, dtype=F64)
    s, t = R.fold_bn(sd["c.conv_s1.bias"], sd["c.bn_s1.running_mean"], sd["c.bn_s1.running_var"], sd["c.bn_s1.weight"], sd["c.bn_s1.bias"])
    assert (s < 0).any()
    got = R.conv3x3_direct_ref(x[:, :4], x[:, 4:], sd["c.conv_s1.weight"], s, t, None, dil, 1, 1, dt=F64)
    assert close12(got, OR._rebnconv(sd, "c.", x, dil))
    w_t = R.conv3x3_weight_t(sd["c.conv_s1.weight"])
    assert w_t.shape == (Cin * 9, Cout) and w_t[2 * 9 + 1 * 3 + 2, 3] == sd["c.conv_s1.weight"][3, 2, 1, 2]


def test_pool_resize_refs_vs_oracle():
    x = -torch.rand(3, 2, 5, 7, generator=R.rng(4), dtype=F64) - 0.5
    assert torch.equal(R.maxpool2_ceil_ref(x, dt=F64), OR._pool(x)) and R.maxpool2_ceil_ref(x, dt=F64).shape[-2:] == (3, 4)
    assert (R.maxpool2_ceil_ref(x, dt=F64) < 0).all()       # a pool that pads with 0 instead of -inf would give 0 in the ragged row / column
    assert close12(R.resize_bilinear_ref(x, 9, 13, 1.0, 0, 0, dt=F64), OR._up(x, torch.empty(1, 1, 9, 13)))
    assert torch.equal(R.resize_bilinear_ref(x, 5, 7, 1.0, 0, 0, dt=F64), x)


def test_instnorm_and_stem_refs_vs_torch():
    x = R.instnorm_input(3, 63, 8, 5)
    want = F.instance_norm(x.double().permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)
    assert close12(R.instnorm_ref(x, 1e-5, 0, dt=F64), want) and close12(R.instnorm_ref(x, 1e-5, 1, dt=F64), want.relu())
    assert torch.equal(R.instnorm_ref(x, 1e-5, 0, dt=F64)[..., 1], torch.zeros(3, 63, dtype=F64))
    one = R.instnorm_ref(R.instnorm_input(1, 1, 8, 6), 1e-5, 0, dt=F64)      # a single spatial element normalises to 0
    assert torch.equal(one, torch.zeros_like(one))
    xs, w, b = R.stem_input(7, 5, 7, True)
    y = F.conv2d(xs.double(), w.double(), b.double(), stride=2, padding=3)
    assert close12(R.conv7x7s2_instnorm_ref(xs, w, b, 1e-5, dt=F64), F.relu(F.instance_norm(y, eps=1e-5)).permute(0, 2, 3, 1))
    assert close12(R.conv7x7s2_ref(xs, w, b, 0, dt=F64), y.permute(0, 2, 3, 1))
    w_t = R.stem_weight_t(w)
    assert w_t.shape == (147, 64) and w_t[2 * 49 + 3 * 7 + 5, 11] == w[11, 2, 3, 5]
    p = R.avgpool2_nhwc_ref(torch.arange(2 * 5 * 7 * 3, dtype=F64).view(2, 5, 7, 3), dt=F64)
    assert p.shape == (2, 2, 3, 3) and p[1, 1, 2, 1] == torch.arange(2 * 5 * 7 * 3, dtype=F64).view(2, 5, 7, 3)[1, 2:4, 4:6, 1].mean()


def test_im2col_ref_column_order():
    x = torch.randn(2, 3, 5, 4, generator=R.rng(7)).half()
    cols = R.im2col3x3_ref(x, 64)
    w = torch.randn(6, 4, 3, 3, generator=R.rng(8), dtype=F64)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, 6)
    w_cols = torch.zeros(6, 64, dtype=F64)
    w_cols[:, :36] = w.permute(0, 2, 3, 1).reshape(6, 36)                   # tap*Cin + c
    assert close12(cols.double() @ w_cols.t(), want) and torch.equal(cols[:, 36:], torch.zeros(30, 28).half())


def test_sentinel_and_excess_helpers():
    s = R.sentinel16(3, 5)
    assert R.is_sentinel16(s) and torch.isnan(s).all()
    s[1, 2] = 0
    assert not R.is_sentinel16(s)
    ref = torch.tensor([1.0, 0.0, -2.0], dtype=F64)
    assert R.elem_excess(ref.clone(), ref, 0.0) == 0.0
    assert R.elem_excess(ref + torch.tensor([2.0 ** -10, 0, 0], dtype=F64), ref, 0.0) == pytest.approx(1.0)
    assert R.elem_excess(ref + torch.tensor([0, 1e-6, 0], dtype=F64), ref, 1e-7) == pytest.approx(10.0)     # one wrong element among many is seen


_CASES = list(R.f16_floor_cases())


def test_every_f16_kernel_has_floor_cases():
    assert {c[0] for c in _CASES} == {"conv7x7s2_c3", "conv7x7s2_instnorm", "instnorm", "dwconv_gelu", "add_act_gelu", "context_split_tanh", "conv1x1_small"}
    assert len({(c[0], c[1]) for c in _CASES}) == len(_CASES)


@pytest.mark.parametrize("kernel", sorted({c[0] for c in _CASES}))
def test_f32_floor_within_cap(kernel):
    """atol = 4 x max|float32 - float64| of every case stays below 2e-3 of the output's RMS (largest per kernel, 4 x included: conv7x7s2_c3 8.0e-6,
    conv7x7s2_instnorm 1.2e-5, instnorm 2.0e-5, dwconv_gelu 8.8e-6, add_act_gelu 3.5e-6, context_split_tanh 1.3e-7, conv1x1_small 1.7e-6)."""
    worst = 0.0
    for name, cid, fn, args in _CASES:
        if name != kernel:
            continue
        atol, rms = R.atol_of(name, cid)
        assert (atol, rms) == R.floor_atol(fn, *args)                       # what the GPU tests import is what is pinned here
        assert atol <= R.ATOL_CAP * rms, (name, cid, atol, rms)
        worst = max(worst, atol)
    print(f"[leaf floor] {kernel}: largest atol {worst:.3e}")
    assert worst < 1e-3
