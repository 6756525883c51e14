"""tests/ip_refs.py pinned to independent forms: the IP term against torch's scaled_dot_product_attention in float64, the image tokens against
nn.Linear / nn.LayerNorm, the block composition against a module-built attention; and the derived bound against a float32 emulation of the kernel's
sequence (the bound must hold for it, with room: it is derived from the formats, not fitted)."""
import math

import pytest
import torch

import ip_refs as R


def _case(d, Tip, seed, B=4, H=8, Tq=9, kv_div=2):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Tq, H * d, generator=g).half()
    kv = torch.randn(B // kv_div, Tip, 2 * H * d, generator=g).half()
    a = torch.randn(B, Tq, H * d, generator=g).half()
    return q, kv, a


@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("Tip", [1, 4, 16])
def test_ip_reference_equals_sdpa(d, Tip):
    B, H, Tq, kv_div = 4, 8, 9, 2
    q, kv, a = _case(d, Tip, 3 + d + Tip)
    scale = 0.6
    got, bound = R.ip_reference(q, kv, a, H, d, d ** -0.5, scale, kv_div)
    qh = q.double().view(B, Tq, H, d).transpose(1, 2)
    idx = torch.arange(B) // kv_div
    k = kv[..., :H * d].double().view(-1, Tip, H, d).transpose(1, 2)[idx]
    v = kv[..., H * d:].double().view(-1, Tip, H, d).transpose(1, 2)[idx]
    o = torch.nn.functional.scaled_dot_product_attention(qh, k, v, scale=d ** -0.5).transpose(1, 2).reshape(B, Tq, H * d)
    want = a.double() + scale * o
    assert (got - want).abs().max().item() < 1e-12
    assert bound.shape == got.shape and (bound > 0).all()
    # the bound is of the size of one f16 rounding: it cannot hide a wrong term
    assert (bound <= 2.0 ** -10 * got.abs() + 1e-3).all()


@pytest.mark.parametrize("d,Tip", [(40, 4), (80, 1), (160, 16)])
def test_bound_holds_for_the_f32_sequence(d, Tip):
    q, kv, a = _case(d, Tip, 11 + d)
    ref, bound = R.ip_reference(q, kv, a, 8, d, d ** -0.5, 0.6, 2)
    emu = R.kernel_sequence_f32(q, kv, a, 8, d, d ** -0.5, 0.6, 2)
    assert ((emu.double() - ref).abs() <= bound).all()
    # and a term that is wrong by one part in 50 is outside it somewhere
    off = R.kernel_sequence_f32(q, kv, a, 8, d, d ** -0.5, 0.6 * 1.02, 2)
    assert ((off.double() - ref).abs() > bound).any()


def test_zero_scale_and_zero_v_leave_a():
    q, kv, a = _case(40, 4, 5)
    assert torch.equal(R.kernel_sequence_f32(q, kv, a, 8, 40, 40 ** -0.5, 0.0, 2), a)
    kv0 = kv.clone()
    kv0[..., 320:] = 0
    assert torch.equal(R.kernel_sequence_f32(q, kv0, a, 8, 40, 40 ** -0.5, 0.6, 2), a)
    ref, _ = R.ip_reference(q, kv0, a, 8, 40, 40 ** -0.5, 0.6, 2)
    assert torch.equal(ref, a.double())


def test_kv_div_picks_the_entry():
    """Samples of the first half read entry 0, of the second half entry 1."""
    q, kv, a = _case(40, 4, 7)
    full, _ = R.ip_reference(q, kv, a, 8, 40, 40 ** -0.5, 1.0, 2)
    for b in range(4):
        one, _ = R.ip_reference(q[b:b + 1], kv[b // 2:b // 2 + 1], a[b:b + 1], 8, 40, 40 ** -0.5, 1.0, 1)
        assert torch.equal(one[0], full[b])


def test_tokens_reference_equals_modules():
    g = torch.Generator().manual_seed(2)
    proj = dict(weight=torch.randn(4 * 768, 1024, generator=g) / 32, bias=0.1 * torch.randn(4 * 768, generator=g),
                norm_weight=1 + 0.1 * torch.randn(768, generator=g), norm_bias=0.1 * torch.randn(768, generator=g))
    emb = torch.randn(1024, generator=g)
    lin, ln = torch.nn.Linear(1024, 4 * 768).double(), torch.nn.LayerNorm(768).double()
    with torch.no_grad():
        lin.weight.copy_(proj["weight"]); lin.bias.copy_(proj["bias"]); ln.weight.copy_(proj["norm_weight"]); ln.bias.copy_(proj["norm_bias"])
        want = torch.stack([ln(lin(torch.zeros(1024, dtype=torch.float64)).view(4, 768)), ln(lin(emb.double()).view(4, 768))])
    got = R.tokens_reference(emb, proj)
    assert got.shape == (2, 4, 768) and (got - want).abs().max().item() < 1e-12
    assert (got[0] - got[1]).abs().max().item() > 0.1            # the zero image's tokens are other tokens


def test_attn2_reference_equals_modules():
    """The block composition against nn.MultiheadAttention-free module code: nn.LayerNorm, nn.Linear and scaled_dot_product_attention."""
    H, C, N, B, Tip = 8, 320, 6, 4, 4
    d = C // H
    g = torch.Generator().manual_seed(4)
    p, t = "blk.", "blk.transformer_blocks.0."
    sd = {t + "norm2.weight": 1 + 0.1 * torch.randn(C, generator=g), t + "norm2.bias": 0.1 * torch.randn(C, generator=g),
          t + "attn2.to_q.weight": torch.randn(C, C, generator=g) / math.sqrt(C), t + "attn2.to_k.weight": torch.randn(C, 768, generator=g) / 28,
          t + "attn2.to_v.weight": torch.randn(C, 768, generator=g) / 28, t + "attn2.to_out.0.weight": torch.randn(C, C, generator=g) / math.sqrt(C),
          t + "attn2.to_out.0.bias": 0.1 * torch.randn(C, generator=g)}
    h, text = torch.randn(B * N, C, generator=g), torch.randn(2, 7, 768, generator=g)
    tokens, w_ip = torch.randn(2, Tip, 768, generator=g), torch.randn(2 * C, 768, generator=g) / 28
    got = R.attn2_reference(sd, p, h, B, N, text, H, tokens, w_ip, 0.6)
    D = torch.float64
    x = h.to(D)
    n = torch.nn.functional.layer_norm(x, (C,), sd[t + "norm2.weight"].to(D), sd[t + "norm2.bias"].to(D))
    q = torch.nn.functional.linear(n, sd[t + "attn2.to_q.weight"].to(D)).view(B, N, H, d).transpose(1, 2)
    out = torch.zeros(B, N, C, dtype=D)
    for b in range(B):
        e = b // 2
        for tok, wk, wv, s in ((text, sd[t + "attn2.to_k.weight"], sd[t + "attn2.to_v.weight"], 1.0), (tokens, w_ip[:C], w_ip[C:], 0.6)):
            k = torch.nn.functional.linear(tok[e].to(D), wk.to(D)).view(-1, H, d).transpose(0, 1)
            v = torch.nn.functional.linear(tok[e].to(D), wv.to(D)).view(-1, H, d).transpose(0, 1)
            out[b] += s * torch.nn.functional.scaled_dot_product_attention(q[b], k, v).transpose(0, 1).reshape(N, C)
    want = x + torch.nn.functional.linear(out.view(B * N, C), sd[t + "attn2.to_out.0.weight"].to(D), sd[t + "attn2.to_out.0.bias"].to(D))
    assert (got - want).abs().max().item() < 1e-11
    off = R.attn2_reference(sd, p, h, B, N, text, H)
    assert (got - off).abs().max().item() > 1e-3


def test_tokens_bound_holds_for_an_f16_emulation():
    """The engine's two f16 roundings emulated on the host (f32 arithmetic between them) lie inside tokens_bound; a swapped entry order does not."""
    g = torch.Generator().manual_seed(6)
    proj = dict(weight=(torch.randn(4 * 768, 1024, generator=g) / 32).half().float(), bias=(0.1 * torch.randn(4 * 768, generator=g)).half().float(),
                norm_weight=(1 + 0.1 * torch.randn(768, generator=g)).half().float(), norm_bias=(0.1 * torch.randn(768, generator=g)).half().float())
    emb = torch.randn(1024, generator=g).half().float()
    ref, bound = R.tokens_reference(emb, proj), R.tokens_bound(emb, proj)
    e = torch.stack([torch.zeros(1024), emb])
    y = (e @ proj["weight"].t() + proj["bias"]).half().float().view(2, 4, 768)
    emu = torch.nn.functional.layer_norm(y, (768,), proj["norm_weight"], proj["norm_bias"], 1e-5).half()
    assert ((emu.double() - ref).abs() <= bound).all() and (bound < 0.05).all()
    assert ((emu.flip(0).double() - ref).abs() > bound).any()
