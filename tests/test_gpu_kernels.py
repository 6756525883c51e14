"""GPU: each path-1 HIP kernel (through the C ABI) against a plain PyTorch fp32 reference of the same op.
Tolerance: inputs are f16, accumulation f32, outputs rounded to f16 -> rel-L2 <= 2e-3 per op."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
H = torch.float16


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@pytest.mark.parametrize("M,N,K", [(1000, 320, 320), (4096, 1280, 640), (300, 960, 320), (77, 64, 768), (129, 2560, 320)])
@pytest.mark.parametrize("act", [0, 1])
def test_gemm(L, M, N, K, act):
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = torch.randn(M, K, device="cuda", generator=g).to(H)
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(H)
    b = torch.randn(N, device="cuda", generator=g).to(H)
    R = torch.randn(M, N, device="cuda", generator=g).to(H)
    C = torch.empty(M, N, device="cuda", dtype=H)
    L.tcl_gemm_f16(A, W, b, R, C, M, N, K, K, K, N, N, act, st())
    ref = A.float() @ W.float().t() + b.float()
    if act:
        ref = F.silu(ref)
    ref = ref + R.float()
    assert rel(C, ref) < 2e-3
    C2 = torch.empty(M, N, device="cuda", dtype=H)
    L.tcl_gemm_f16(A, W, 0, 0, C2, M, N, K, K, K, N, N, 0, st())
    assert rel(C2, A.float() @ W.float().t()) < 2e-3


@pytest.mark.parametrize("B,Hh,Ww,Cin,Cout,stride,pad,up", [
    (2, 18, 24, 64, 128, 1, 1, None), (3, 23, 30, 128, 64, 2, 1, None), (2, 12, 15, 64, 64, 1, 1, (23, 30)),
    (2, 9, 10, 64, 320, 1, 1, (18, 20)), (2, 16, 24, 64, 64, 2, 0, None),
    (2, 1, 3, 64, 64, 1, 1, (1, 6)), (2, 3, 1, 64, 64, 1, 1, (6, 1)), (2, 1, 1, 128, 64, 1, 1, (1, 2))])     # up-sampling along one axis only (yt planes of <= 4 frames)
def test_conv3x3(L, B, Hh, Ww, Cin, Cout, stride, pad, up):
    g = torch.Generator(device="cuda").manual_seed(Cin + Cout + Hh)
    x = torch.randn(B, Cin, Hh, Ww, device="cuda", generator=g).to(H)
    w = (torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / (9 * Cin) ** 0.5).to(H)
    b = torch.randn(Cout, device="cuda", generator=g).to(H)
    xin = x.float()
    if up:
        xin = F.interpolate(xin, size=up, mode="nearest")
    if pad == 0:
        xin = F.pad(xin, (0, 1, 0, 1))
    ref = F.conv2d(xin, w.float(), b.float(), stride=stride, padding=pad)
    Ho, Wo = ref.shape[-2:]
    x_nhwc = x.permute(0, 2, 3, 1).contiguous()
    w_t = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
    y = torch.empty(B, Ho, Wo, Cout, device="cuda", dtype=H)
    L.tcl_conv3x3_f16(x_nhwc, w_t, b, 0, y, B, Hh, Ww, Cin, Cout, stride, pad, up[0] if up else 0, up[1] if up else 0, 0, st())
    assert rel(y.permute(0, 3, 1, 2), ref) < 2e-3


def ws_bytes(n):
    return torch.empty(int(n), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("C1,C2,silu", [(320, 0, 1), (640, 320, 1), (1280, 640, 0), (128, 0, 1)])
def test_groupnorm(L, C1, C2, silu):
    g = torch.Generator(device="cuda").manual_seed(C1)
    B, HW = 3, 23 * 30
    x1 = (torch.randn(B, HW, C1, device="cuda", generator=g) * 2 + 0.5).to(H)
    x2 = torch.randn(B, HW, C2, device="cuda", generator=g).to(H) if C2 else None
    C = C1 + C2
    ga, be = torch.randn(C, device="cuda", generator=g).to(H), torch.randn(C, device="cuda", generator=g).to(H)
    y = torch.empty(B, HW, C, device="cuda", dtype=H)
    ws = torch.zeros(int(L.tcl_groupnorm_workspace_bytes(B, C)), dtype=torch.uint8, device="cuda")   # zeroed once by the caller
    for _ in range(3):        # successive calls alternate the two statistics slots; each clears the other one
        y.zero_()
        L.tcl_groupnorm_f16(x1, C1, x2 if C2 else 0, C2, ga, be, y, B, HW, 32, 1e-5, silu, ws, st())
    x = torch.cat([x1, x2], -1) if C2 else x1
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, ga.float(), be.float(), 1e-5).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    assert rel(y, ref) < 2e-3


def test_layernorm_geglu_softmax_gemv(L):
    g = torch.Generator(device="cuda").manual_seed(1)
    for C in (320, 640, 1280):
        x = (torch.randn(999, C, device="cuda", generator=g) * 3).to(H)
        ga, be = torch.randn(C, device="cuda", generator=g).to(H), torch.randn(C, device="cuda", generator=g).to(H)
        y = torch.empty_like(x)
        L.tcl_layernorm_f16(x, ga, be, y, 999, C, 1e-5, st())
        assert rel(y, F.layer_norm(x.float(), (C,), ga.float(), be.float(), 1e-5)) < 2e-3
        # norm1 of a VidToMe-patched block writes the matching metric as well: same y, and the metric the matching would have computed
        # from y itself (tcl_tome_normalize_f16), bit for bit -- the maps cannot depend on which kernel normalised
        y2, m2, m = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        L.tcl_layernorm_metric_f16(x, ga, be, y2, m2, 999, C, 1e-5, st())
        L.tcl_tome_normalize_f16(y, m, 999, C, st())
        assert torch.equal(y2, y) and torch.equal(m2, m)
    x = torch.randn(500, 2560, device="cuda", generator=g).to(H)
    y = torch.empty(500, 1280, device="cuda", dtype=H)
    L.tcl_geglu_f16(x, y, 500, 1280, st())
    assert rel(y, x[:, :1280].float() * F.gelu(x[:, 1280:].float())) < 2e-3
    s = (torch.randn(77, 1000, device="cuda", generator=g) * 4).to(H)
    ref = torch.softmax(s.float() * 0.3, -1)
    L.tcl_softmax_rows_f16(s, 77, 1000, 1000, 0.3, st())
    assert rel(s, ref) < 2e-3
    W = (torch.randn(1280, 320, device="cuda", generator=g) / 18).to(H)
    v, b, a = (torch.randn(n, device="cuda", generator=g).to(H) for n in (320, 1280, 1280))
    o = torch.empty(1280, device="cuda", dtype=H)
    L.tcl_gemv_f16(W, v, b, a, o, 1280, 320, 1, 0, st())
    assert rel(o, (W.float() @ F.silu(v.float()).to(H).float() + b.float()).to(H).float() + a.float()) < 2e-3
    te = torch.empty(320, device="cuda", dtype=H)
    L.tcl_timestep_embed_f16(801.0, 320, te, st())
    fr = torch.exp(-torch.log(torch.tensor(10000.0)) * torch.arange(160) / 160)
    ref = torch.cat([torch.cos(801.0 * fr), torch.sin(801.0 * fr)])
    assert (te.cpu().float() - ref).abs().max() < 2e-3


@pytest.mark.parametrize("d,B,Tq,Tk,kv_div", [(40, 2, 300, 300, 1), (40, 2, 1000, 777, 1), (80, 4, 260, 154, 2), (160, 2, 180, 180, 1),
                                             (80, 2, 129, 64, 1), (40, 2, 64, 2113, 1), (40, 16, 1793, 200, 1)])
def test_attention(L, d, B, Tq, Tk, kv_div):
    Hh = 8
    C = Hh * d
    g = torch.Generator(device="cuda").manual_seed(d + Tq)
    q = torch.randn(B, Tq, C, device="cuda", generator=g).to(H)
    k = torch.randn(B // kv_div, Tk, C, device="cuda", generator=g).to(H)
    v = torch.randn(B // kv_div, Tk, C, device="cuda", generator=g).to(H)
    o = torch.zeros(B, Tq, C, device="cuda", dtype=H)
    wq, wkv = ws_bytes(L.tcl_attention_q_bytes(B, Hh, Tq, d)), ws_bytes(L.tcl_attention_kv_bytes(B // kv_div, Hh, Tk, d))
    L.tcl_attention_f16(q, C, Tq * C, k, C, Tk * C, v, C, Tk * C, o, C, Tq * C, B, Hh, Tq, Tk, d, d ** -0.5, kv_div, 1, wq, wkv, st())
    qq = q.float().view(B, Tq, Hh, d).transpose(1, 2)
    kk = k.float().view(-1, Tk, Hh, d).transpose(1, 2).repeat_interleave(kv_div, 0)
    vv = v.float().view(-1, Tk, Hh, d).transpose(1, 2).repeat_interleave(kv_div, 0)
    ref = F.scaled_dot_product_attention(qq, kk, vv).transpose(1, 2).reshape(B, Tq, C)
    assert rel(o, ref) < 3e-3
    # strided fused-QKV input + reuse of packed K/V
    o2 = torch.zeros_like(o)
    L.tcl_attention_f16(q, C, Tq * C, 0, 0, 0, 0, 0, 0, o2, C, Tq * C, B, Hh, Tq, Tk, d, d ** -0.5, kv_div, 0, wq, wkv, st())
    assert torch.equal(o, o2)
    # the packing half on its own (tcl_attention_pack_f16, possibly on another stream) + the attention kernels alone (pack_kv bit 2): same bits
    wq3, wkv3 = ws_bytes(L.tcl_attention_q_bytes(B, Hh, Tq, d)), ws_bytes(L.tcl_attention_kv_bytes(B // kv_div, Hh, Tk, d))
    o3 = torch.zeros_like(o)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.tcl_attention_pack_f16(q, C, Tq * C, k, C, Tk * C, v, C, Tk * C, B, Hh, Tq, Tk, d, d ** -0.5, kv_div, 1, wq3, wkv3, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    L.tcl_attention_f16(q, C, Tq * C, 0, 0, 0, 0, 0, 0, o3, C, Tq * C, B, Hh, Tq, Tk, d, d ** -0.5, kv_div, 4, wq3, wkv3, st())
    assert torch.equal(o, o3)


def test_pack_unpack_adain(L):
    g = torch.Generator(device="cuda").manual_seed(3)
    N, h, w = 7, 10, 12
    x = torch.randn(N, 4, h, w, device="cuda", generator=g).to(H)
    c = torch.randn(N, 4, h, w, device="cuda", generator=g).to(H)
    idx = torch.tensor([5, 1, 2], dtype=torch.int32, device="cuda")
    out = torch.empty(6, h, w, 8, device="cuda", dtype=H)
    L.tcl_pack_latents_f16(x, c, idx, 3, 0, 0, 0, h, w, out, st())
    ref = torch.cat([x[idx.long()], c[idx.long()]], 1).permute(0, 2, 3, 1)
    assert torch.equal(out[:3], ref) and torch.equal(out[3:], ref)
    cols = torch.tensor([11, 0, 4, 7], dtype=torch.int32, device="cuda")
    sl, nwin = 2, 5
    out = torch.empty(8, nwin, h, 8, device="cuda", dtype=H)
    L.tcl_pack_latents_f16(x, c, cols, 4, 1, sl, nwin, h, w, out, st())
    xt = torch.cat([x, c], 1)[sl:sl + nwin][:, :, :, cols.long()].permute(3, 1, 0, 2)   # 'n c h w -> w c n h'
    assert torch.equal(out[:4], xt.permute(0, 2, 3, 1))
    eps = torch.randn(8, nwin, h, 4, device="cuda", generator=g).to(H)
    noise = torch.zeros(N, 4, h, w, device="cuda", dtype=H)
    L.tcl_unpack_cfg_f16(eps, cols, 4, 1, sl, nwin, h, w, 2.0, sl + 2, 0.5 ** 0.5, nwin, noise, st())
    e = eps.float().permute(0, 3, 1, 2)                                                    # [2F, c, n, h]
    pred = e[:4] + 2.0 * (e[4:] - e[:4])                                                   # w c n h
    refn = torch.zeros(N, 4, h, w, device="cuda")
    refn[sl:sl + nwin][:, :, :, cols.long()] = pred.permute(2, 1, 3, 0)
    refn[sl:sl + 2] *= 0.5 ** 0.5
    assert (noise.float() - refn).abs().max() < 4e-3
    a, b = torch.randn(N, 4, h, w, device="cuda", generator=g).to(H), (torch.randn(N, 4, h, w, device="cuda", generator=g) * 2 + 1).to(H)
    a0, b0 = a.float(), b.float()
    L.tcl_adain_fuse_f16(a, b, N * 4, h * w, 0.01, st())
    def ms(t):
        return t.flatten(2).mean(2)[..., None, None], (t.flatten(2).var(2) + 1e-5).sqrt()[..., None, None]
    ma, sa = ms(a0); mb, sb = ms(b0)
    ra = (a0 - ma) / sa * sb + mb
    assert rel(a, ra) < 2e-3 and rel(b, 0.1 * ra + 0.99 ** 0.5 * b0) < 2e-3


def test_scheduler_vs_oracle(L):
    from oracle.scheduler import Scheduler as OS
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    n = 20
    sch, osch = DPMSolverSDEScheduler(), OS(n)
    sch.set_timesteps(n)
    assert sch.timesteps.tolist() == osch.timesteps.tolist() and sch.timesteps[0] > 990 and sch.timesteps[-1] <= 5
    ac = np.cumprod(1 - np.linspace(0.00085, 0.012, 1000))                           # 'linear' betas (model_utils.py:71-78)
    assert abs(float(sch.sigmas[0]) - ((1 - ac[-1]) / ac[-1]) ** 0.5) < 1e-3 and sch.sigmas[-1] == 0
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 4, 8, 8, generator=g) * float(sch.sigmas[0])
    xd, xo = x.cuda().half(), x.half().float()
    for i in range(n):
        eps, z = torch.randn(3, 4, 8, 8, generator=g).half(), torch.randn(3, 4, 8, 8, generator=g).half()
        sch.step(eps.cuda(), sch.timesteps[i], xd, noise=z.cuda())
        xo = osch.step(eps, xo, z).half().float()
        assert rel(xd.cpu(), xo) < 2e-3, (i, rel(xd.cpu(), xo))


def test_vidtome_maps_vs_oracle(L):
    """Same f16 tokens -> HIP matching vs the oracle's f16-emulating rule: every token must be restored from the same representative
    except where f32 accumulation order flips an f16 rounding (rare)."""
    from oracle import vidtome as OV
    from tc_light_amd.vidtome import VidToMe
    g = np.random.default_rng(3)
    N, C = 345, 320
    tome = VidToMe("cuda")
    bank = None
    serial, table, ids_h, ids_o = 0, {}, None, None
    for F, randf, coin in [(4, 2, 0.9), (3, 0, 0.7), (4, 1, 0.1), (1, -1, 0.3)]:
        base = g.standard_normal((1, N, C)).astype(np.float32)
        x = torch.from_numpy(base + 0.3 * g.standard_normal((2 * F, N, C)).astype(np.float32)).half()
        tome.draws = [(randf, coin)]
        tome.begin_forward(F, (15, 23))
        tome.trace = []
        merged, unm, T = tome.compute_merge("blk", x.cuda(), F, N, C)
        assert merged.index is None and merged.entry_stride == T * C and merged.block.is_contiguous()
        merged = merged.block
        r = OV.compute_merge(x.float(), F, bank, randf, coin, emulate_f16=True)
        assert T == r["merged"].shape[1]
        um = unm.cpu().long() if unm is not None else torch.arange(F * N)
        # slot numbering of the unmerged tokens is free (attention is permutation-invariant; the HIP path keeps them in index order, the
        # reference in score order): compare what every token is RESTORED from, i.e. unmerge applied to the merged tokens themselves
        mh = merged.cpu().float()
        rest_h, rest_o = mh[:, um], r["merged"][:, r["unm"]]
        agree = (rest_h == rest_o).all(-1).float().mean().item()
        assert agree > 0.995, agree
        # provenance bookkeeping of the whole-path tests (tests/e2e_oracle.py): ids carried through the engine's recorded maps / the oracle's
        # dict must name exactly the tokens the restored VALUES come from, banks included
        import e2e_oracle as E
        serial += 1
        ids = (serial << 32) + torch.arange(F * N, dtype=torch.int64)
        for i_, v_ in zip(ids.tolist(), x.float().reshape(2, F * N, C)[0]):
            table[i_] = v_
        sh, ids_h = E.trace_provenance(tome.trace[-1], ids, ids_h)
        so, ids_o = E.oracle_provenance(r, ids, ids_o)
        assert torch.equal(rest_h[0], torch.stack([table[i_] for i_ in sh.tolist()]))
        assert torch.equal(rest_o[0], torch.stack([table[i_] for i_ in so.tolist()]))
        assert torch.equal(tome.banks["blk"].cpu().float()[0], torch.stack([table[i_] for i_ in ids_h.tolist()]))
        assert abs((sh == so).float().mean().item() - agree) < 2e-3
        ids_o = ids_h.clone()                        # (the oracle continues from the HIP bank below)
        if agree == 1.0:
            # the merged SET must match as well
            hv = torch.from_numpy(g.standard_normal(C).astype(np.float32))
            a, b = (mh @ hv).sort(-1).values, (r["merged"] @ hv).sort(-1).values
            assert torch.equal(a, b)
            assert torch.equal((tome.banks["blk"].cpu().float() @ hv).sort(-1).values, (r["bank_new"] @ hv).sort(-1).values)   # same bank, as a set
        bank = tome.banks["blk"].cpu().float()       # continue the chain from the HIP bank so later rounds stay comparable


def _tome_chain_case(L, passes, size, N, C, ne, with_metric, lazy, **kw):
    """One chain of chunks (passes: begin_step by begin_step, each chunk (F, randf or one per round, coin)) through VidToMe and through the
    materialised reference chain (tests/tome_chain_ref.py) on the same tokens: T, merged rows, unm, bank and every trace entry must be EQUAL."""
    from tc_light_amd.vidtome import VidToMe
    from tome_chain_ref import ChainRef
    g = np.random.default_rng(11)
    xs = [[torch.from_numpy(g.standard_normal((1, N, C)).astype(np.float32) + 0.3 * g.standard_normal((2 * F, N, C)).astype(np.float32)).half().cuda()
           for F, _, _ in ps] for ps in passes]
    tome, ref = VidToMe("cuda", **kw), ChainRef("cuda", **kw)
    tome.trace = []
    k = 0
    for ps, xp in zip(passes, xs):
        tome.draws = [(rf, coin) for _, rf, coin in ps]
        tome.begin_step([F for F, _, _ in ps], size)
        for i, ((F, rf, coin), x) in enumerate(zip(ps, xp)):
            tome.select_chunk(i)
            xin = x[:F].contiguous() if ne == 1 else x
            met = None
            if with_metric:
                met = torch.empty_like(xin)
                L.tcl_tome_normalize_f16(xin, met, xin.shape[0] * N, C, st())
            merged, unm, T = tome.compute_merge("blk", xin, F, N, C, metric=met, ne=ne, lazy_merged=lazy)
            src, sbs, idx = merged
            assert lazy or (idx is None and src.is_contiguous() and src.shape == (ne, T, C) and sbs == T * C)
            rows = torch.stack([torch.as_strided(src, (T if idx is None else src.shape[1], C), (C, 1), src.storage_offset() + b * sbs) for b in range(ne)])
            m1 = rows if idx is None else rows[:, idx.long()]
            m0, u0, T0 = ref.compute_merge("blk", xin, F, list(rf) if isinstance(rf, (list, tuple)) else [rf], coin, N, C, metric=met, ne=ne)
            b1, b0 = tome.banks.get("blk"), ref.banks.get("blk")
            assert T == T0 and torch.equal(m1, m0), (kw, ne, with_metric, lazy, k)
            assert (b1 is None and b0 is None) or torch.equal(b1, b0), (kw, ne, with_metric, lazy, k)
            assert (unm is None and u0 is None) or torch.equal(unm, u0), (kw, ne, with_metric, lazy, k)
            k += 1
    torch.cuda.synchronize()
    assert len(tome.trace) == len(ref.trace)
    for a_, b_ in zip(tome.trace, ref.trace):
        assert a_.keys() == b_.keys()
        for key in a_:
            va, vb = a_[key], b_[key]
            assert (torch.equal(va, vb) if isinstance(va, torch.Tensor) else va == vb), key
    return k


def test_vidtome_chain_equals_materialised_reference(L):
    """compute_merge carries the cosine-normalised rows beside the tokens and writes local survivors / banks straight into the next [src | dst]
    block (no `cat` copy, no second normalisation).  Every map, merged sequence and bank must equal those of the chain that materialises every stage
    (tests/tome_chain_ref.py: gather -> cat -> normalise -> match) BIT FOR BIT, over a multi-chunk pass in which the next chunk's layout is
    planned ahead (begin_step with all chunks), with and without norm1's metric, with one and two batch entries, lazy and materialised merged
    sequences, and across a pass boundary (a second begin_step meeting the bank the first one left) -- and on the branches TC-Light's own configs
    leave idle: several randframe rounds (F = 8, 16: two rounds, unm_pre > 0 in the second), per-sample maps (align_batch=False) and no global
    merge, each a chain of chunks that meets its own bank (the chains of test_vidtome_multi_round_and_per_sample_vs_oracle; N = 150 keeps
    nb >= 128, so single rounds still take the strip kernel)."""
    passes = [[(4, 2, 0.9), (3, 0, 0.7), (4, 1, 0.1), (1, -1, 0.3), (2, 1, 0.8)], [(4, 3, 0.2), (4, 0, 0.6)]]
    for ne, with_metric, lazy in ((2, True, True), (2, False, False), (1, True, True), (2, True, False)):
        assert _tome_chain_case(L, passes, (15, 23), 345, 320, ne, with_metric, lazy) == 7
    for C, kw, chain in ((320, dict(align_batch=True), [(8, [3, 0], 0.9), (8, [1, 1], 0.2), (6, [2], 0.7), (16, [0, 3], 0.4), (4, [1], 0.8)]),
                         (640, dict(align_batch=False), [(4, [2], 0.9), (4, [0], 0.1), (8, [3, 0], 0.6), (1, [], 0.3), (3, [1], 0.7)]),
                         (320, dict(merge_global=False), [(4, [1], 0.5), (8, [2, 1], 0.5), (1, [], 0.5)])):
        for with_metric, lazy in ((False, False), (True, True)):
            assert _tome_chain_case(L, [chain], (10, 15), 150, C, 2, with_metric, lazy, **kw) == len(chain)      # one pass: every next chunk is planned for
            assert _tome_chain_case(L, [[c] for c in chain], (10, 15), 150, C, 2, with_metric, lazy, **kw) == len(chain)      # a pass per chunk: none is


def _restored(merged, unm, F, N):
    """unmerge applied to the merged tokens themselves: [2, F*N, C] (slot numbering of the unmerged tokens is free, see above)."""
    if unm is None:
        return merged
    if unm.dim() == 1:
        return merged[:, unm]
    return torch.stack([merged[b, unm[b]] for b in range(2)])


def test_vidtome_multi_round_and_per_sample_vs_oracle(L):
    """The two compute_merge branches TC-Light's own configs leave idle: chunks of more than target_stride frames
    (several randframe rounds, 8 -> 2 -> 1 and 16 -> 4 -> 1, patch.py:43-56) and per-sample matching (align_batch=False, merge.py:109-118).
    Same f16 tokens -> HIP path vs the oracle's f16-emulating rule (the oracle itself is pinned bit-exactly to the reference's
    compute_merge on these branches: tests/test_oracle_path1.py)."""
    from oracle import vidtome as OV
    from tc_light_amd.vidtome import VidToMe
    g = np.random.default_rng(17)
    N = 150
    for C, aligned, chain in ((320, True, [(8, [3, 0], 0.9), (8, [1, 1], 0.2), (6, [2], 0.7), (16, [0, 3], 0.4), (4, [1], 0.8)]),
                              (640, False, [(4, [2], 0.9), (4, [0], 0.1), (8, [3, 0], 0.6), (1, [], 0.3), (3, [1], 0.7)])):
        tome = VidToMe("cuda", align_batch=aligned)
        bank = None
        for F, randfs, coin in chain:
            base = g.standard_normal((1, N, C)).astype(np.float32)
            x = torch.from_numpy(base + 0.3 * g.standard_normal((2 * F, N, C)).astype(np.float32)).half()
            tome.draws = [(randfs, coin)]
            tome.begin_forward(F, (10, 15))
            merged, unm, T = tome.compute_merge("blk", x.cuda(), F, N, C)
            assert merged.index is None and merged.entry_stride == T * C and merged.block.is_contiguous()
            merged = merged.block
            r = OV.compute_merge(x.float(), F, bank, randfs, coin, emulate_f16=True, align_batch=aligned)
            assert T == r["merged"].shape[1], (F, T, r["merged"].shape)
            assert r["rounds"] == len(randfs)
            if unm is not None and not aligned:
                assert unm.dim() == 2
            mh = merged.cpu().float()
            rest_h = _restored(mh, unm.cpu().long() if unm is not None else None, F, N)
            rest_o = _restored(r["merged"], r["unm"], F, N)
            agree = (rest_h == rest_o).all(-1).float().mean().item()
            assert agree > 0.99, (C, aligned, F, agree)
            if agree == 1.0:
                # same merged SET and same bank, as sets of rows: an exact integer hash of each row's f16 bit pattern (a float dot product
                # with a random vector is not bit-stable across row positions in the CPU BLAS)
                hw_ = torch.from_numpy(g.integers(1, 1 << 20, C)).long()
                rh = lambda t: (t.half().view(torch.int16).long() * hw_).sum(-1).sort(-1).values
                assert torch.equal(rh(mh), rh(r["merged"]))
                assert torch.equal(rh(tome.banks["blk"].cpu().float()), rh(r["bank_new"]))
            # unmerge_add = residual + unmerge, per sample
            h = torch.zeros(2 * F * N, C, dtype=H, device="cuda")
            y = torch.randn(2, T, C, device="cuda").to(H)
            tome.unmerge_add(h, F * N * C, y, T, unm, F * N, C)
            want = _restored(y.cpu().float(), unm.cpu().long() if unm is not None else None, F, N).reshape(2 * F * N, C)
            assert torch.equal(h.cpu().float(), want)
            bank = tome.banks["blk"].cpu().float()
    torch.cuda.synchronize()


def test_splitk_gemm_conv(L):
    """small-M deep-K problems take the split-K path once a workspace is registered; result must match the direct path."""
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    M, N, K = 384, 1280, 11520
    A = torch.randn(M, K, device="cuda", generator=g).to(H)
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(H)
    b, R = torch.randn(N, device="cuda", generator=g).to(H), torch.randn(M, N, device="cuda", generator=g).to(H)
    C0, C1 = torch.empty(M, N, device="cuda", dtype=H), torch.empty(M, N, device="cuda", dtype=H)
    L.tcl_set_workspace(0, 0)
    L.tcl_gemm_f16(A, W, b, R, C0, M, N, K, K, K, N, N, 1, st())
    L.tcl_set_workspace(ws, ws.numel())
    L.tcl_gemm_f16(A, W, b, R, C1, M, N, K, K, K, N, N, 1, st())
    ref = F.silu(A.float() @ W.float().t() + b.float()) + R.float()
    assert rel(C1, ref) < 2e-3 and rel(C0, ref) < 2e-3
    x = torch.randn(8, 4, 12, 1280, device="cuda", generator=g).to(H)
    w = (torch.randn(1280, 9 * 1280, device="cuda", generator=g) / 107).to(H)
    y0, y1 = torch.empty(8, 4, 12, 1280, device="cuda", dtype=H), torch.empty(8, 4, 12, 1280, device="cuda", dtype=H)
    L.tcl_conv3x3_f16(x, w, b, 0, y1, 8, 4, 12, 1280, 1280, 1, 1, 0, 0, 0, st())
    L.tcl_set_workspace(0, 0)
    L.tcl_conv3x3_f16(x, w, b, 0, y0, 8, 4, 12, 1280, 1280, 1, 1, 0, 0, 0, st())
    assert rel(y1, y0) < 1e-3
    torch.cuda.synchronize()


def test_gemm_fused_geglu(L):
    from tc_light_amd.unet import _geglu_rows
    g = torch.Generator(device="cuda").manual_seed(11)
    M, C = 777, 320
    A = torch.randn(M, C, device="cuda", generator=g).to(H)
    W = (torch.randn(8 * C, C, device="cuda", generator=g) / C ** 0.5).to(H)
    b = torch.randn(8 * C, device="cuda", generator=g).to(H)
    out = torch.empty(M, 4 * C, device="cuda", dtype=H)
    L.tcl_gemm_f16(A, _geglu_rows(W).contiguous(), _geglu_rows(b).contiguous(), 0, out, M, 8 * C, C, C, C, 4 * C, 8 * C, 2, st())
    f = A.float() @ W.float().t() + b.float()
    assert rel(out, f[:, :4 * C] * F.gelu(f[:, 4 * C:])) < 2e-3


@pytest.mark.parametrize("shape", [("g", 5520, 1280, 1280), ("g", 21600, 640, 640), ("g", 1472, 1280, 2560), ("g", 33333, 960, 320),
                                   ("g", 20001, 352, 320), ("c", 8, 23, 30, 640, 640), ("c", 8, 4, 12, 1280, 1280),
                                   ("g", 9001, 384, 640), ("c", 3, 40, 56, 128, 128)])
def test_gemm_configs_bit_identical(L, shape):
    """Every tile configuration (LDS-DMA 128x128 / 64x128 / 128x64 / 64x64 / 256x128, the 8-wave 256x320 / 128x320 / 256x256 /
    128x256 kernels, the round-4 8-phase 256x256 / 256x320 / 512x128 kernels of csrc/gemm8q.hip -- cfg 13 / 14 / 15, 16x16x32 MFMAs with the weight
    fragment as the row operand; for K = 320 the strip-resident Linear of csrc/linstrip.hip, cfg 12, whose MFMA operand roles are swapped)
    accumulates each output in the same k order, so with equal K splits the results are bit-identical -- the property the automatic
    configuration choice relies on -- and the automatic choice itself matches them."""
    ws = torch.empty(96 << 20, dtype=torch.uint8, device="cuda")
    L.tcl_set_workspace(ws, ws.numel())
    g = torch.Generator(device="cuda").manual_seed(3)
    if shape[0] == "g":
        _, M, N, K = shape
        A = torch.randn(M, K, device="cuda", generator=g).to(H)
        W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(H)
        b, R = torch.randn(N, device="cuda", generator=g).to(H), torch.randn(M, N, device="cuda", generator=g).to(H)

        def run():
            C = torch.empty(M, N, device="cuda", dtype=H)
            L.tcl_gemm_f16(A, W, b, R, C, M, N, K, K, K, N, N, 0, st())
            return C
        ref = A.float() @ W.float().t() + b.float() + R.float()
    else:
        _, B, Hh, Ww, Ci, Co = shape
        x = torch.randn(B, Hh, Ww, Ci, device="cuda", generator=g).to(H)
        w = (torch.randn(Co, 9 * Ci, device="cuda", generator=g) / (9 * Ci) ** 0.5).to(H)
        b = torch.randn(Co, device="cuda", generator=g).to(H)

        def run():
            y = torch.empty(B, Hh, Ww, Co, device="cuda", dtype=H)
            L.tcl_conv3x3_f16(x, w, b, 0, y, B, Hh, Ww, Ci, Co, 1, 1, 0, 0, 0, st())
            return y
        ref = F.conv2d(x.permute(0, 3, 1, 2).float(), w.view(Co, 3, 3, Ci).permute(0, 3, 1, 2).float(), b.float(), padding=1).permute(0, 2, 3, 1)
    try:
        for splits in (1, 4):
            outs = {}
            for cfg in (1, 2, 3, 4, 11, 5, 6, 7, 8, 12, 13, 14, 15):
                if splits > 1 and cfg in (5, 6, 7, 8, 12, 13, 14, 15):
                    continue
                L.tcl_gemm_tune(cfg, splits)
                try:
                    outs[cfg] = run()
                except RuntimeError:          # configuration not applicable to this shape
                    continue
            assert len(outs) >= 4 and (splits > 1 or shape[0] != "g" or shape[3] != 320 or 12 in outs)
            first = next(iter(outs.values()))
            assert rel(first, ref) < 2e-3
            for cfg, o in outs.items():
                assert torch.equal(o, first), f"cfg {cfg} splits {splits} differs"
        L.tcl_gemm_tune(0, 0)
        auto1, auto2 = run(), run()            # first call tunes, second hits the cache
        assert torch.equal(auto1, auto2) and rel(auto1, ref) < 2e-3
    finally:
        L.tcl_gemm_tune(0, 0)
        L.tcl_set_workspace(0, 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["silu", "gelu_after_resid", "k64", "k128", "k320_small_m", "geglu", "conv_s2", "conv_s2_pad0", "conv_silu_resid", "n128_silu_resid", "conv_n128_s2_pad0",
                                  "conv_up_23x40", "conv_up_2x", "conv_up_one_axis"])
def test_gemm8q_epilogues_and_tails_equal_tiled_kernels(L, case):
    """The 8-phase kernels (cfg 13 = 256x256, 14 = 256x320, 15 = 512x128; csrc/gemm8q.hip) against the LDS-DMA tile kernel (cfg 1) and the round-3 8-wave
    kernel (cfg 7, GEGLU) on what test_gemm_configs_bit_identical does not reach: every epilogue (SiLU, GELU after the residual, GEGLU in
    registers), K = one / two / five K tiles (prologue and tail paths of the two-buffer ring), fewer rows than one tile, stride-2 convolutions
    with symmetric and with the VAE encoder's asymmetric padding (tap masks), a convolution with activation + residual, nearest up-sampling
    fused in the gather (12x20 -> 23x40: not a factor 2; exact 2x; one axis only, as the yt planes of short windows produce).  Bit equality."""
    g = torch.Generator(device="cuda").manual_seed(11)
    mk = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc).to(H)
    ref_cfg = 1
    if case in ("silu", "gelu_after_resid", "k64", "k128", "k320_small_m", "geglu", "n128_silu_resid"):
        M, N, K, act, hasr = {"silu": (3000, 1280, 640, 1, False), "gelu_after_resid": (2049, 1280, 1280, 5, True), "k64": (777, 1280, 64, 0, True),
                              "k128": (1025, 1280, 128, 4, False), "k320_small_m": (100, 1280, 320, 0, True), "geglu": (2500, 2560, 320, 2, False),
                              "n128_silu_resid": (5000, 128, 448, 1, True)}[case]
        A, W, b = mk(M, K), mk(N, K, sc=K ** -0.5), mk(N)
        R = mk(M, N) if hasr else None
        No = N // 2 if act == 2 else N
        if act == 2:
            ref_cfg = 7

        def run():
            C = torch.empty(M, No, device="cuda", dtype=H)
            L.tcl_gemm_f16(A, W, b, R if hasr else 0, C, M, N, K, K, K, No, N, act, st())
            return C
        cfgs = (13,) if act == 2 else ((15,) if N == 128 else (13, 14))
    else:
        up = {"conv_up_23x40": (23, 40), "conv_up_2x": (20, 32), "conv_up_one_axis": (3, 12)}.get(case)
        B, Hh, Ww, Ci, Co, stride, pad, act, hasr = {"conv_s2": (3, 46, 30, 640, 640, 2, 1, 0, False),
                                                     "conv_up_23x40": (3, 12, 20, 640, 1280, 1, 1, 0, False), "conv_up_2x": (2, 10, 16, 256, 256, 1, 1, 0, True),
                                                     "conv_up_one_axis": (40, 3, 6, 640, 640, 1, 1, 0, False), "conv_s2_pad0": (2, 40, 56, 256, 256, 2, 0, 0, False),
                                                     "conv_silu_resid": (5, 23, 30, 320, 640, 1, 1, 1, True),
                                                     "conv_n128_s2_pad0": (2, 44, 60, 128, 128, 2, 0, 0, False)}[case]
        Hu, Wu = up if up else (Hh, Ww)
        Ho = (Hu + 2 - 3) // stride + 1 if pad else (Hu + 1 - 3) // stride + 1
        Wo = (Wu + 2 - 3) // stride + 1 if pad else (Wu + 1 - 3) // stride + 1
        x, w, b = mk(B, Hh, Ww, Ci), mk(Co, 9 * Ci, sc=(9 * Ci) ** -0.5), mk(Co)
        R = mk(B, Ho, Wo, Co) if hasr else None

        def run():
            y = torch.empty(B, Ho, Wo, Co, device="cuda", dtype=H)
            L.tcl_conv3x3_f16(x, w, b, R if hasr else 0, y, B, Hh, Ww, Ci, Co, stride, pad, up[0] if up else 0, up[1] if up else 0, act, st())
            return y
        cfgs = (13, 14) if Co % 1280 == 0 else ((13,) if Co % 256 == 0 else (14,))
        if Co == 640:
            cfgs = (14,)
        if Co == 128:
            cfgs = (15,)
    try:
        L.tcl_gemm_tune(ref_cfg, 1)
        ref = run()
        for cfg in cfgs:
            L.tcl_gemm_tune(cfg, 1)
            out = run()
            assert torch.isfinite(out.float()).all()
            assert torch.equal(out, ref), f"{case}: cfg {cfg} differs from cfg {ref_cfg} in {(out != ref).sum().item()} of {out.numel()} outputs (max |d| {(out.float() - ref.float()).abs().max().item():.3e})"
    finally:
        L.tcl_gemm_tune(0, 0)
    torch.cuda.synchronize()


def test_ln_gemm_fused(L):
    """LayerNorm folded into the strip-resident K = 320 Linear (tcl_ln_gemm_f16) against tcl_layernorm_f16 + tcl_gemm_f16 and against torch f32:
    plain, bias + SiLU, GEGLU; M not a multiple of the 128-row strip."""
    from tc_light_amd.unet import _geglu_rows
    g = torch.Generator(device="cuda").manual_seed(21)
    M, C = 20011, 320
    x = (torch.randn(M, C, device="cuda", generator=g) * 2 + 0.3).to(H)
    ga, be = (1 + 0.2 * torch.randn(C, device="cuda", generator=g)).to(H), (0.1 * torch.randn(C, device="cuda", generator=g)).to(H)
    y = torch.empty_like(x)
    L.tcl_layernorm_f16(x, ga, be, y, M, C, 1e-5, st())
    ref_ln = F.layer_norm(x.float(), (C,), ga.float(), be.float(), 1e-5)
    for N, act, has_b in ((320, 0, False), (960, 1, True), (2560, 2, True)):
        W = (torch.randn(N, C, device="cuda", generator=g) / C ** 0.5).to(H)
        b = torch.randn(N, device="cuda", generator=g).to(H) if has_b else None
        Wk, bk = (_geglu_rows(W).contiguous(), _geglu_rows(b).contiguous()) if act == 2 else (W, b)
        No = N // 2 if act == 2 else N
        two, one = torch.empty(M, No, device="cuda", dtype=H), torch.empty(M, No, device="cuda", dtype=H)
        L.tcl_gemm_f16(y, Wk, bk if bk is not None else 0, 0, two, M, N, C, C, C, No, N, act, st())
        L.tcl_ln_gemm_f16(x, ga, be, 1e-5, Wk, bk if bk is not None else 0, 0, one, M, N, C, C, C, No, N, act, st())
        f = ref_ln @ W.float().t() + (b.float() if b is not None else 0)
        ref = f[:, :N // 2] * F.gelu(f[:, N // 2:]) if act == 2 else (F.silu(f) if act == 1 else f)
        assert rel(one, ref) < 2e-3 and rel(one, two.float()) < 1e-3, (N, act, rel(one, ref), rel(one, two.float()))
        assert (one != two).float().mean().item() < 0.02          # same rounding points: only rows whose statistics differ in the last bit move


def test_ln_gemm_qpanel_equals_linear_then_pack(L):
    """Round 5: the attn2 to_q projection written straight into the flash kernel's query panel (tcl_ln_gemm_qpanel_f16) must leave the SAME BITS in the
    panel as tcl_ln_gemm_f16 followed by the pack pass of tcl_attention_pack_f16 -- and never touch the panel's padding rows; the attention that
    follows (pre-packed Q, text K / V packed earlier) then equals the unfused call bit for bit.  Tq = 345 (panel rows padded to 512), 3 samples,
    the last strip of 128 rows partly past M."""
    g = torch.Generator(device="cuda").manual_seed(33)
    B, Hh, d, Tq, Lt = 3, 8, 40, 345, 154
    C, M = Hh * d, 3 * 345
    x = (torch.randn(M, C, device="cuda", generator=g) * 1.5 + 0.2).to(H)
    ga, be = (1 + 0.2 * torch.randn(C, device="cuda", generator=g)).to(H), (0.1 * torch.randn(C, device="cuda", generator=g)).to(H)
    W = (torch.randn(C, C, device="cuda", generator=g) / C ** 0.5).to(H)
    kv = torch.randn(B, Lt, 2 * C, device="cuda", generator=g).to(H)
    nq, nkv = L.tcl_attention_q_bytes(B, Hh, Tq, d), L.tcl_attention_kv_bytes(B, Hh, Lt, d)
    # the two-step route
    q = torch.empty(M, C, device="cuda", dtype=H)
    L.tcl_ln_gemm_f16(x, ga, be, 1e-5, W, 0, 0, q, M, C, C, C, C, C, C, 0, st())
    wq_a, wkv = torch.zeros(nq, dtype=torch.uint8, device="cuda"), torch.empty(nkv, dtype=torch.uint8, device="cuda")
    L.tcl_attention_pack_f16(q, C, Tq * C, kv, 2 * C, Lt * 2 * C, kv[:, :, C:], 2 * C, Lt * 2 * C, B, Hh, Tq, Lt, d, d ** -0.5, 1, 1, wq_a, wkv, st())
    o_a = torch.empty(M, C, device="cuda", dtype=H)
    L.tcl_attention_f16(q, C, Tq * C, 0, 0, 0, 0, 0, 0, o_a, C, Tq * C, B, Hh, Tq, Lt, d, d ** -0.5, 1, 4, wq_a, wkv, st())
    # the fused route, into a panel whose padding rows carry a sentinel pattern of zeros
    wq_b = torch.zeros(nq, dtype=torch.uint8, device="cuda")
    L.tcl_ln_gemm_qpanel_f16(x, ga, be, 1e-5, W, M, Hh, d, Tq, C, C, d ** -0.5, wq_b, st())
    o_b = torch.empty(M, C, device="cuda", dtype=H)
    L.tcl_attention_f16(wq_b, C, Tq * C, 0, 0, 0, 0, 0, 0, o_b, C, Tq * C, B, Hh, Tq, Lt, d, d ** -0.5, 1, 4, wq_b, wkv, st())
    torch.cuda.synchronize()
    Tqp = (Tq + 255) // 256 * 256
    pa = wq_a[:B * Hh * Tqp * 48 * 2].view(H).view(B, Hh, Tqp, 48)
    pb = wq_b[:B * Hh * Tqp * 48 * 2].view(H).view(B, Hh, Tqp, 48)
    assert torch.equal(pa[:, :, :Tq], pb[:, :, :Tq])                       # same bits in every written row, padding columns 40..47 zero in both
    assert (pb[:, :, Tq:] == 0).all() and (pb[..., 40:] == 0).all()
    assert torch.equal(o_a, o_b)
    ref = F.scaled_dot_product_attention(*(t.float().view(B, -1, Hh, d).transpose(1, 2) for t in (q.view(B, Tq, C), kv[:, :, :C], kv[:, :, C:]))).transpose(1, 2).reshape(M, C)
    assert rel(o_b, ref) < 3e-3


@pytest.mark.parametrize("d,T,ne", [(40, 345, 2), (40, 1411, 2), (80, 333, 2), (40, 777, 1), (80, 64, 1)])
def test_gemm_qkv_panels_equal_gemm_then_pack(L, d, T, ne):
    """Round 5: attn1's QKV projection written straight into the Q / K / V^T panels (tcl_gemm_qkv_panels_f16: M tiles per batch entry, Q / K row chunks
    re-addressed, V transposed through the staged C tile with the panel's key permutation, skew and ones row) against tcl_gemm_f16 +
    tcl_attention_pack_f16: EVERY byte of the three panels equal -- lengths that are no multiple of 64 / 128 / 256, an entry boundary inside an M tile of
    the plain GEMM, a single entry (the CFG pair's shared prefix) -- and the attention on them bit-identical."""
    g = torch.Generator(device="cuda").manual_seed(100 + d + T)
    Hh = 8
    C = Hh * d
    x = torch.randn(ne * T, C, device="cuda", generator=g).to(H)
    W = (torch.randn(3 * C, C, device="cuda", generator=g) / C ** 0.5).to(H)
    nq, nkv = L.tcl_attention_q_bytes(ne, Hh, T, d), L.tcl_attention_kv_bytes(ne, Hh, T, d)
    qkv = torch.empty(ne * T, 3 * C, device="cuda", dtype=H)
    L.tcl_gemm_f16(x, W, 0, 0, qkv, ne * T, 3 * C, C, C, C, 3 * C, 3 * C, 0, st())
    wq_a, wkv_a = torch.zeros(nq, dtype=torch.uint8, device="cuda"), torch.zeros(nkv, dtype=torch.uint8, device="cuda")
    L.tcl_attention_pack_f16(qkv, 3 * C, T * 3 * C, qkv[:, C:], 3 * C, T * 3 * C, qkv[:, 2 * C:], 3 * C, T * 3 * C, ne, Hh, T, T, d, d ** -0.5, 1, 1, wq_a, wkv_a, st())
    wq_b, wkv_b = torch.zeros(nq, dtype=torch.uint8, device="cuda"), torch.zeros(nkv, dtype=torch.uint8, device="cuda")
    for _ in range(2):                                           # twice into the same workspace: the second call must leave the same bytes
        L.tcl_gemm_qkv_panels_f16(x, T * C, 0, W, ne, T, Hh, d, C, C, C, d ** -0.5, wq_b, wkv_b, st())
    # the same through a row index: the merged tokens as rows idx[t] of a larger per-entry source block (the VidToMe merge map in the operand load)
    Ts = T + 57
    idx = torch.randperm(Ts, device="cuda", generator=g)[:T].to(torch.int32).contiguous()
    src = torch.randn(ne, Ts, C, device="cuda", generator=g).to(H)
    src[:, idx.long()] = x.view(ne, T, C)
    wq_c, wkv_c = torch.zeros(nq, dtype=torch.uint8, device="cuda"), torch.zeros(nkv, dtype=torch.uint8, device="cuda")
    L.tcl_gemm_qkv_panels_f16(src, Ts * C, idx, W, ne, T, Hh, d, C, C, C, d ** -0.5, wq_c, wkv_c, st())
    torch.cuda.synchronize()
    assert torch.equal(wq_c[:ne * Hh * ((T + 255) // 256 * 256) * ((d + 15) // 16 * 16) * 2], wq_b[:ne * Hh * ((T + 255) // 256 * 256) * ((d + 15) // 16 * 16) * 2]) and torch.equal(wkv_c, wkv_b), "row-index form"
    Tqp, DP = (T + 255) // 256 * 256, (d + 15) // 16 * 16
    nqp = ne * Hh * Tqp * DP * 2
    assert torch.equal(wq_a[:nqp], wq_b[:nqp]), "Q panel"
    assert torch.equal(wkv_a, wkv_b), "K / V^T panels"
    oa, ob = torch.empty(ne * T, C, device="cuda", dtype=H), torch.empty(ne * T, C, device="cuda", dtype=H)
    L.tcl_attention_f16(qkv, 3 * C, T * 3 * C, 0, 0, 0, 0, 0, 0, oa, C, T * C, ne, Hh, T, T, d, d ** -0.5, 1, 4, wq_a, wkv_a, st())
    L.tcl_attention_f16(wq_b, 3 * C, T * 3 * C, 0, 0, 0, 0, 0, 0, ob, C, T * C, ne, Hh, T, T, d, d ** -0.5, 1, 4, wq_b, wkv_b, st())
    assert torch.equal(oa, ob)
    q, k, v = (qkv[:, i * C:(i + 1) * C].float().view(ne, T, Hh, d).transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(ne * T, C)
    assert rel(ob, ref) < 3e-3


def test_gemm_fused_geglu_configs(L):
    """GEGLU epilogue (64-row [32 value | 32 gate] groups) across tile configurations, incl. the 8-wave 256x256 / 128x256 kernels."""
    from tc_light_amd.unet import _geglu_rows
    g = torch.Generator(device="cuda").manual_seed(12)
    M, C = 4100, 320
    A = torch.randn(M, C, device="cuda", generator=g).to(H)
    W = (torch.randn(8 * C, C, device="cuda", generator=g) / C ** 0.5).to(H)
    b = torch.randn(8 * C, device="cuda", generator=g).to(H)
    Wg, bg = _geglu_rows(W).contiguous(), _geglu_rows(b).contiguous()
    f = A.float() @ W.float().t() + b.float()
    ref = f[:, :4 * C] * F.gelu(f[:, 4 * C:])
    outs = {}
    try:
        for cfg in (1, 2, 3, 4, 11, 7, 8, 12):
            L.tcl_gemm_tune(cfg, 1)
            out = torch.empty(M, 4 * C, device="cuda", dtype=H)
            L.tcl_gemm_f16(A, Wg, bg, 0, out, M, 8 * C, C, C, C, 4 * C, 8 * C, 2, st())
            outs[cfg] = out
            assert rel(out, ref) < 2e-3, cfg
        first = outs[1]
        for cfg, o in outs.items():
            assert torch.equal(o, first), cfg
    finally:
        L.tcl_gemm_tune(0, 0)
