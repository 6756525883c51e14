"""Float64 restatements for generation.ip_adapter (IP-Adapter, Ye et al. 2023): the image tokens, the decoupled image cross-attention term that
tcl_attention_ip_add_f16 adds to the text attention's output, the attn2 of a transformer block with it, and the per-element error bound of the kernel.
Pinned to independent forms (torch's scaled_dot_product_attention, nn.LayerNorm, nn.Linear) by tests/test_ip_refs_cpu.py.

The bound.  The kernel (include/tclight_hip.h) works on the f16 operands widened to f32, every operation rounded to f32 on its own (u = 2^-24,
gamma_n = n u / (1 - n u)), and rounds the result to f16 once.  With R the float64 value of a_i + ip_scale * sum_t w_t v_ti from the same f16 operands:
  scores     s_t = qk_scale * sum_i q_i k_ti is a sequential sum of d products and one more product: |s^_t - s_t| <= gamma_(d+2) * A_t,
             A_t = qk_scale * sum_i |q_i k_ti|  (the absolute sum);
  exponent   the argument s_t - m carries the errors of s_t and of the maximum and one rounding: D = 2 max_t(gamma_(d+2) A_t) + u max_t |s_t - m|;
             expf is accurate to 2 ulp (the HIP math library documents 1), so each e_t has relative error rho = (exp(D) - 1) + 4 u;
  weights    l sums Tip terms (gamma_(Tip-1)), w_t = e_t / l is one more rounding: relative error rho_w = 2 rho + gamma_(Tip+1), times 1.01 for the
             second-order terms;
  V sum      Tip products and sums: |o^_i - o_i| <= (rho_w + gamma_(Tip+1)) * sum_t |w_t v_ti|  (the absolute sum);
  result     ip_scale * o and the addition are one rounding each: E32 = ip_scale * (that) + u |ip_scale o_i| + u |R|;
  f16        one rounding of the f32 result: 2^-11 (|R| + E32), or half the subnormal spacing 2^-25.
bound = E32 + 2^-11 (|R| + E32) + 2^-25.  It depends on the operands and on d and Tip alone, not on what the kernel returns.
"""
import math

import torch

U32 = 2.0 ** -24


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def _split(kv, H, d):
    """kv [E, Tip, 2*H*d] -> (K, V) [E, H, Tip, d] float64."""
    E, Tip, _ = kv.shape
    k = kv[..., :H * d].double().view(E, Tip, H, d).permute(0, 2, 1, 3)
    v = kv[..., H * d:].double().view(E, Tip, H, d).permute(0, 2, 1, 3)
    return k, v


def ip_term(q, kv, H, d, qk_scale, kv_div):
    """q [B, Tq, H*d], kv [B / kv_div, Tip, 2*H*d] (K | V) -> (term, bound pieces) in float64:
    term [B, Tq, H*d] = softmax(q K^T * qk_scale) V per (sample, head), sample b reading entry b // kv_div."""
    B, Tq, C = q.shape
    qh = q.double().view(B, Tq, H, d).permute(0, 2, 1, 3)                           # [B, H, Tq, d]
    k, v = _split(kv, H, d)
    idx = torch.arange(B) // kv_div
    k, v = k[idx], v[idx]                                                           # [B, H, Tip, d]
    s = qh @ k.transpose(-1, -2) * qk_scale                                         # [B, H, Tq, Tip]
    sabs = qh.abs() @ k.abs().transpose(-1, -2) * abs(qk_scale)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    w = e / e.sum(-1, keepdim=True)
    o = w @ v                                                                       # [B, H, Tq, d]
    oabs = w @ v.abs()
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, Tq, C)
    spread = (s - m).abs().max(-1).values                                           # [B, H, Tq]
    return back(o), dict(oabs=back(oabs), amax=sabs.max(-1).values, spread=spread, Tip=kv.shape[1], d=d, H=H)


def ip_reference(q, kv, a, H, d, qk_scale, ip_scale, kv_div):
    """-> (R, bound), float64 [B, Tq, H*d]: the value tcl_attention_ip_add_f16 leaves in `a` and the per-element bound derived above."""
    o, p = ip_term(q, kv, H, d, qk_scale, kv_div)
    R = a.double() + ip_scale * o
    B, Tq, C = o.shape
    Tip = p["Tip"]
    D = 2.0 * gamma(d + 2) * p["amax"] + U32 * p["spread"]                          # [B, H, Tq]
    rho = torch.expm1(D) + 4.0 * U32
    rho_w = 1.01 * (2.0 * rho + gamma(Tip + 1))
    per_head = (rho_w + gamma(Tip + 1)).permute(0, 2, 1)[..., None].expand(B, Tq, H, d).reshape(B, Tq, C)
    e32 = abs(ip_scale) * per_head * p["oabs"] + U32 * (ip_scale * o).abs() + U32 * R.abs()
    bound = e32 + 2.0 ** -11 * (R.abs() + e32) + 2.0 ** -25
    return R, bound


def kernel_sequence_f32(q, kv, a, H, d, qk_scale, ip_scale, kv_div):
    """The kernel's float sequence emulated on the host in float32 (sums in index order, no contraction) -> f16 [B, Tq, H*d].  torch's exp stands in
    for expf: the emulation checks the bound, it is not a bit reference."""
    B, Tq, C = q.shape
    Tip = kv.shape[1]
    f32 = torch.float32
    qh = q.float().view(B, Tq, H, d)
    idx = torch.arange(B) // kv_div
    k = kv[..., :C].float().view(-1, Tip, H, d)[idx]                                # [B, Tip, H, d]
    v = kv[..., C:].float().view(-1, Tip, H, d)[idx]
    s = torch.zeros(B, Tq, H, Tip, dtype=f32)
    for i in range(d):
        s = s + qh[..., i][..., None] * k[..., i].permute(0, 2, 1)[:, None]        # [B, Tq, H, Tip]
    s = s * torch.tensor(qk_scale, dtype=f32)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e[..., 0]
    for t in range(1, Tip):
        l = l + e[..., t]
    w = e / l[..., None]
    o = torch.zeros(B, Tq, H, d, dtype=f32)
    for t in range(Tip):
        o = o + w[..., t][..., None] * v[:, t][:, None]
    term = torch.tensor(ip_scale, dtype=f32) * o.reshape(B, Tq, C)
    out = (a.float() + term).half()
    return torch.where(term == 0, a.half(), out)


def tokens_reference(embeds, proj, n_tokens=4, eps=1e-5):
    """embeds [1024] -> [2, n_tokens, 768] float64: entry 0 from the zero embedding, entry 1 from `embeds`; LayerNorm(proj(e).view(n_tokens, 768))."""
    e = torch.stack([torch.zeros_like(embeds.double()), embeds.double()])
    y = e @ proj["weight"].double().t() + proj["bias"].double()
    y = y.view(2, n_tokens, -1)
    mu, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
    return (y - mu) / torch.sqrt(var + eps) * proj["norm_weight"].double() + proj["norm_bias"].double()


def tokens_bound(embeds, proj, n_tokens=4, eps=1e-5):
    """Per-element bound of ip_adapter.image_tokens against tokens_reference on the same (f16-valued) operands -> float64 [2, n_tokens, 768].
    The engine rounds twice to f16: y = f16(e W^T + bias) out of the GEMM (f32 accumulation over K = 1024 products and the bias) and the LayerNorm's
    output (f32 arithmetic on the f16 y).
      GEMM        |dy_i| <= 2^-11 |y_i| + gamma_(K+2) (sum_k |e_k W_ik| + |bias_i|) =: D_i, and D = max_i D_i over the token's row;
      LayerNorm   out_i = g_i (y_i - mu) / sigma + b_i.  A perturbation dy moves y_i - mu by at most 2 D and sigma by at most D (the standard
                  deviation is 1-Lipschitz in the max norm), so to first order |d out_i| <= |g_i| / sigma (2 + |yhat_i|) D, yhat = (y - mu) / sigma;
                  times 1.05 for the second-order terms (D / sigma is about 2e-3 here);
      its own f32 arithmetic (two sums over 768 terms, a handful of products): gamma_(768+8) (|g_i yhat_i| + |b_i|);
      f16         2^-11 (|out_i| + the above) + 2^-25."""
    e = torch.stack([torch.zeros_like(embeds.double()), embeds.double()])
    W, b = proj["weight"].double(), proj["bias"].double()
    y = e @ W.t() + b
    D = 2.0 ** -11 * y.abs() + gamma(W.shape[1] + 2) * (e.abs() @ W.abs().t() + b.abs())
    y, D = y.view(2, n_tokens, -1), D.view(2, n_tokens, -1).max(-1, keepdim=True).values
    mu, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
    sigma = torch.sqrt(var + eps)
    yhat = (y - mu) / sigma
    g, bb = proj["norm_weight"].double(), proj["norm_bias"].double()
    out = yhat * g + bb
    e32 = 1.05 * g.abs() / sigma * (2.0 + yhat.abs()) * D + gamma(y.shape[-1] + 8) * ((g * yhat).abs() + bb.abs())
    return e32 + 2.0 ** -11 * (out.abs() + e32) + 2.0 ** -25


def attn2_reference(sd, p, h, B, N, text, H, ip_tokens=None, ip_weight=None, ip_scale=0.0):
    """attn2 of transformer block `p` of the UNet state dict `sd` in float64: h [B*N, C] -> h + to_out(Attention(q, text) [+ ip_scale *
    Attention(q, image tokens)]), q = to_q(norm2(h)).  text [2, L, 768] and ip_tokens [2, Tip, 768]: entry 0 for the first half of the samples.
    ip_weight [2C, 768] = to_k_ip ; to_v_ip."""
    t = p + "transformer_blocks.0."
    g = lambda k: sd[t + k].double()
    C = h.shape[1]
    d = C // H
    x = h.double()
    n = torch.nn.functional.layer_norm(x, (C,), g("norm2.weight"), g("norm2.bias"), 1e-5)
    q = (n @ g("attn2.to_q.weight").t()).view(B, N, H, d).permute(0, 2, 1, 3)
    idx = torch.arange(B) // (B // 2)

    def attend(tokens, wk, wv):
        k = (tokens.double() @ wk.t()).view(2, -1, H, d).permute(0, 2, 1, 3)[idx]
        v = (tokens.double() @ wv.t()).view(2, -1, H, d).permute(0, 2, 1, 3)[idx]
        w = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
        return (w @ v).permute(0, 2, 1, 3).reshape(B * N, C)
    o = attend(text, g("attn2.to_k.weight"), g("attn2.to_v.weight"))
    if ip_tokens is not None:
        o = o + ip_scale * attend(ip_tokens, ip_weight[:C].double(), ip_weight[C:].double())
    return x + o @ g("attn2.to_out.0.weight").t() + g("attn2.to_out.0.bias")
