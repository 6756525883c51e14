"""generation.ip_adapter on the GPU: tcl_attention_ip_add_f16 against the float64 restatement and its derived bound (tests/ip_refs.py), attn2 of one
block per channel width against the float64 composition of the block's own weights, the UNet pass and the Generator's loop with and without it."""
import os

import pytest
import torch

import ip_refs as R

pytestmark = pytest.mark.gpu

B, H, TQ, KV_DIV, PAD, GUARD = 4, 8, 70, 2, 16, 64
SENT = 0x7E01                                     # a NaN bit pattern no arithmetic produces: padding and guards must keep it


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def _strided(vals, ld):
    """vals [B, TQ, C] f16 (host) -> (device buffer, view [B, TQ, ld] inside it): rows ld > C wide, the padding and GUARD halves on both sides SENT."""
    n = vals.shape[0] * vals.shape[1] * ld
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int16).view(torch.float16).cuda()
    view = buf[GUARD:GUARD + n].view(vals.shape[0], vals.shape[1], ld)
    view[..., :vals.shape[2]] = vals.cuda()
    return buf, view


def _untouched(buf, view, C):
    bits = buf.view(torch.int16)
    n = view.numel()
    pad = view[..., C:].contiguous().view(torch.int16)
    return bool((bits[:GUARD] == SENT).all() and (bits[GUARD + n:] == SENT).all() and (pad == SENT).all())


_CASES = {}


def case(d, Tip):
    """Operands and the float64 reference of one (d, Tip): made once, shared by the tests and left unchanged."""
    if (d, Tip) not in _CASES:
        g = torch.Generator().manual_seed(100 * d + Tip)
        C = H * d
        q = torch.randn(B, TQ, C, generator=g).half()
        kv = torch.randn(B // KV_DIV, Tip, 2 * C, generator=g).half()
        a = torch.randn(B, TQ, C, generator=g).half()
        ref, bound = R.ip_reference(q, kv, a, H, d, d ** -0.5, 0.6, KV_DIV)
        _CASES[(d, Tip)] = dict(q=q, kv=kv, a=a, ref=ref, bound=bound)
    return _CASES[(d, Tip)]


def run_kernel(L, c, d, Tip, scale, kv=None):
    C = H * d
    ld = C + PAD
    qb, qv = _strided(c["q"], ld)
    ab, av = _strided(c["a"], ld)
    kvd = (c["kv"] if kv is None else kv).cuda().contiguous()
    L.tcl_attention_ip_add_f16(qv, ld, TQ * ld, kvd, av, ld, TQ * ld, B, H, TQ, Tip, d, d ** -0.5, scale, KV_DIV, st())
    torch.cuda.synchronize()
    assert _untouched(ab, av, C) and _untouched(qb, qv, C), "padding or guard halves were written"
    assert torch.equal(qv[..., :C].cpu(), c["q"]), "q was written"
    return av[..., :C].cpu()


@pytest.mark.parametrize("Tip", [1, 4, 16])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_kernel_within_bound_of_float64(L, d, Tip):
    c = case(d, Tip)
    got = run_kernel(L, c, d, Tip, 0.6)
    err = (got.double() - c["ref"]).abs()
    worst = (err / c["bound"]).max().item()
    print(f"d={d} Tip={Tip}: max |err| {err.max().item():.3e}, max err/bound {worst:.3f}, moved {(got != c['a']).float().mean().item():.3f} of the elements")
    assert torch.isfinite(got.float()).all()
    assert (err <= c["bound"]).all(), f"max err/bound {worst}"
    assert (got != c["a"]).float().mean().item() > 0.5           # the term really is added
    again = run_kernel(L, c, d, Tip, 0.6)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))


@pytest.mark.parametrize("Tip", [1, 4, 16])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_kernel_zero_scale_and_zero_v_keep_the_bits(L, d, Tip):
    c = case(d, Tip)
    a = c["a"].clone()
    a[0, 0, :8] = torch.tensor([-0.0, 0.0, 6e-8, -6e-8, 65504.0, -65504.0, 1.0, -1.0]).half()      # signed zeros, subnormals, the largest
    c2 = dict(c, a=a)
    zero = run_kernel(L, c2, d, Tip, 0.0)
    assert torch.equal(zero.view(torch.int16), a.view(torch.int16))
    kv0 = c["kv"].clone()
    kv0[..., H * d:] = 0
    v0 = run_kernel(L, c2, d, Tip, 0.6, kv=kv0)
    assert torch.equal(v0.view(torch.int16), a.view(torch.int16))


def test_kernel_refuses_bad_arguments_before_a_launch(L):
    d, Tip = 40, 4
    c = case(d, Tip)
    C = H * d
    q, kv, a = c["q"].cuda(), c["kv"].cuda(), c["a"].cuda()
    big = torch.randn(B // KV_DIV, 17, 2 * C).half().cuda()
    ok = dict(q=q, ldq=C, qbs=TQ * C, kv=kv, lda=C, abs_=TQ * C, B=B, H=H, Tq=TQ, Tip=Tip, d=d, kv_div=KV_DIV)
    bad = [dict(Tip=0), dict(Tip=17, kv=big), dict(d=64), dict(d=0), dict(kv_div=3), dict(kv_div=0), dict(ldq=C + 4), dict(lda=C - 8), dict(q=0), dict(kv=0)]
    for change in bad:
        k = dict(ok, **change)
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_attention_ip_add_f16(k["q"], k["ldq"], k["qbs"], k["kv"], a, k["lda"], k["abs_"], k["B"], k["H"], k["Tq"], k["Tip"], k["d"],
                                       k["d"] ** -0.5 if k["d"] else 1.0, 0.6, k["kv_div"], st())
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):        # a bad argument is refused at scale 0 too
        L.tcl_attention_ip_add_f16(q, C, TQ * C, kv, a, C, TQ * C, B, H, TQ, 0, d, d ** -0.5, 0.0, KV_DIV, st())
    torch.cuda.synchronize()
    assert torch.equal(a.cpu().view(torch.int16), c["a"].view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- block and engine
@pytest.fixture(scope="module")
def unet(L):
    from tc_light_amd import ip_adapter as IP
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    sd = sd15.random_state_dict(sd15.unet_param_shapes(), seed=1)
    tome = VidToMe("cuda", seed=5)
    eng = UNetEngine(sd, "cuda", tome)
    _, weights = IP.check_state(IP.seeded_state_dict(3))
    g = torch.Generator().manual_seed(17)
    tokens = torch.randn(2, 4, 768, generator=g).half()
    return dict(sd=sd, eng=eng, tome=tome, weights=weights, tokens=tokens)


def prompt(unet, scale, zero_v=False):
    from tc_light_amd import ip_adapter as IP
    w = unet["weights"]
    if zero_v:
        w = {p: torch.cat([t[:t.shape[0] // 2], torch.zeros_like(t[t.shape[0] // 2:])]) for p, t in w.items()}
    return IP.make_prompt(unet["tokens"], w, scale, "cuda")


@pytest.mark.parametrize("p", ["down_blocks.0.attentions.0.", "down_blocks.1.attentions.1.", "mid_block.attentions.0."])
def test_block_attn2_against_float64(unet, p):
    """attn2 of one block per channel width (320, 640, 1280), N = 35 tokens (no multiple of a tile), against the float64 composition of the block's
    own weights as the engine holds them (f16).  The error with the image tokens may be at most twice the error without them, on the same inputs:
    the term adds one f16-rounded addend of comparable size to the attention output; the error without is the existing code's and is measured here."""
    eng, sd = unet["eng"], unet["sd"]
    C = eng.tfm[p]["c"]
    Bq, N, scale = 4, 35, 0.6
    g = torch.Generator().manual_seed(C)
    h = torch.randn(Bq * N, C, generator=g).half()
    text = torch.randn(2, 77, 768, generator=g).half().cuda()
    sd16 = {k: v.half() for k, v in sd.items() if k.startswith(p + "transformer_blocks.0.")}
    w_ip = unet["weights"][p].half()
    ref_off = R.attn2_reference(sd16, p, h, Bq, N, text.cpu(), 8)
    ref_on = R.attn2_reference(sd16, p, h, Bq, N, text.cpu(), 8, unet["tokens"], w_ip, scale)
    off = eng.attn2(p, h.cuda(), Bq, N, text).double().cpu()
    on = eng.attn2(p, h.cuda(), Bq, N, text, ip=prompt(unet, scale)).double().cpu()
    torch.cuda.synchronize()
    rel = lambda x, r: ((x - r).norm() / r.norm()).item()
    e_off, e_on = rel(off, ref_off), rel(on, ref_on)
    print(f"{p} C={C}: rel-L2 vs float64 without ip {e_off:.3e}, with ip {e_on:.3e} (ratio {e_on / e_off:.2f}); the term moves the output by "
          f"{rel(on, off):.3e}")
    assert torch.isfinite(on).all() and rel(ref_on, ref_off) > 1e-3              # the references differ: the term is not negligible
    assert e_on <= 2.0 * e_off


HH, WW, T_STEP, FS, DRAWS = 8, 12, 601.0, [2, 2], [(1, 0.9), (0, 0.2)]


def _pass(unet, x, text, ip):
    eng, tome = unet["eng"], unet["tome"]
    tome.reset_global_tokens()
    outs = []
    for _ in range(2):                                          # the second pass meets packed text K / V (ip=None: the fused query-panel route)
        tome.draws = list(DRAWS)
        outs.append(eng.forward_many(x, FS, HH, WW, T_STEP, text, cfg_pair=True, ip=ip).clone())
    tome.reset_global_tokens()
    tome.draws = None
    torch.cuda.synchronize()
    return outs


def test_engine_pass_with_and_without(unet):
    g = torch.Generator(device="cuda").manual_seed(31)
    xh = torch.randn(sum(FS), HH, WW, 8, device="cuda", generator=g).half()
    x = torch.cat([xh, xh]).contiguous()
    text = torch.randn(2, 77, 768, device="cuda", generator=g).half()
    base = _pass(unet, x, text, None)
    for name, ip in (("scale 0", prompt(unet, 0.0)), ("zero to_v_ip", prompt(unet, 0.6, zero_v=True))):
        got = _pass(unet, x, text, ip)
        for a, b in zip(got, base):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), name
    ip = prompt(unet, 0.6)
    on, again = _pass(unet, x, text, ip), _pass(unet, x, text, ip)
    for a, b, c in zip(on, again, base):
        assert torch.isfinite(a.float()).all() and torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert not torch.equal(a, c) and (a.float() - c.float()).abs().max().item() > 1e-3
    with pytest.raises(ValueError, match="down_blocks.0.attentions.0."):          # a weight of another block's width is refused by name
        from tc_light_amd.unet import ImagePrompt
        wrong = dict(ip.weights, **{"down_blocks.0.attentions.0.": ip.weights["mid_block.attentions.0."]})
        eng_ip = ImagePrompt(ip.tokens, wrong, 0.6)
        unet["eng"].forward_many(x, FS, HH, WW, T_STEP, text, cfg_pair=True, ip=eng_ip)


class Recorder:
    """The launch trace hook of tests/test_gpu_unet_trace.py: stands in for the ctypes library object and notes the name of every call, with the
    kind of pass (xy / yt) it was issued in."""

    def __init__(self, real):
        self.real, self.calls, self.where = real, [], "xy"

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*a):
            self.calls.append((self.where, name))
            return fn(*a)
        return call


def test_generator_loop(unet):
    """4 frames of 64x64, 2 steps, multi-axis on: scale 0 is the run without the key bit for bit; scale 0.6 differs, is finite and repeats; the new
    kernel is launched by the xy passes (16 blocks per UNet call) and by no yt pass."""
    from tc_light_amd.generate import Generator
    eng, tome = unet["eng"], unet["tome"]
    n, hh, ww = 4, 8, 8
    cfg = dict(n_timesteps=2, alpha_t=0.3, final_factor_t=0.5, win_size_t=4, chunk_size=2, guidance_scale=2.0, seed=77, max_tokens_per_pass=1 << 20)
    gen = torch.Generator().manual_seed(3)
    conds, conds_t = torch.randn(2, 77, 768, generator=gen).half().cuda(), torch.randn(2, 77, 768, generator=gen).half().cuda()
    cc = torch.randn(n, 4, hh, ww, generator=gen).half().cuda()
    block = dict(image="reference.png", scale=0.6, path=None)
    state = tome.rng.bit_generator.state
    rec = Recorder(eng.L)

    def run(config, ip, record=False):
        tome.rng.bit_generator.state = state
        tome.reset_global_tokens()
        g = Generator(eng, None, config, image_prompt=ip)
        g.prepare_data(torch.zeros(n, 3, 8 * hh, 8 * ww, device="cuda"))
        if record:
            yt = g._unet_yt

            def marked(*a, **k):
                rec.where = "yt"
                try:
                    return yt(*a, **k)
                finally:
                    rec.where = "xy"
            g._unet_yt = marked
            eng.L = eng.ops.L = rec
        try:
            x = g.ddim_sample(g.init_noise.clone(), conds, conds_t, cc).clone()
        finally:
            eng.L = eng.ops.L = rec.real
        torch.cuda.synchronize()
        return x

    with pytest.raises(ValueError, match="generation.ip_adapter"):
        Generator(eng, None, dict(cfg, ip_adapter=block))                        # the key without its tokens is not silently ignored
    plain = run(cfg, None)
    zero = run(dict(cfg, ip_adapter=dict(block, scale=0.0)), prompt(unet, 0.0))
    assert torch.equal(plain.view(torch.int16), zero.view(torch.int16))
    on = run(dict(cfg, ip_adapter=block), prompt(unet, 0.6), record=True)
    again = run(dict(cfg, ip_adapter=block), prompt(unet, 0.6))
    assert torch.isfinite(on.float()).all() and torch.equal(on.view(torch.int16), again.view(torch.int16))
    assert not torch.equal(on, plain)
    name = "tcl_attention_ip_add_f16"
    xy = sum(1 for w, f in rec.calls if f == name and w == "xy")
    yt = sum(1 for w, f in rec.calls if f == name and w == "yt")
    yt_unets = sum(1 for w, f in rec.calls if f == "tcl_im2col3x3_small_f16" and w == "yt")
    xy_unets = sum(1 for w, f in rec.calls if f == "tcl_im2col3x3_small_f16" and w == "xy")
    print(f"launches of {name}: {xy} in {xy_unets} xy UNet calls, {yt} in {yt_unets} yt UNet calls")
    assert yt_unets >= 2 and yt == 0 and xy_unets >= 2 and xy == 16 * xy_unets


# ---------------------------------------------------------------------------------------------------------------- the image tokens, layer by layer
TINY = dict(embed_dim=1024, image_resolution=28, vision_layers=2, vision_width=64, vision_patch_size=14, context_length=8, vocab_size=50,
            transformer_width=64, transformer_layers=1)              # a CLIP of ViT-H/14's interface (patch 14, 1024-d image_embeds) at toy size
TINY_KW = dict(vision_heads=1, act="gelu", crop="floor")
TINY_VISION_CONFIG = dict(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1, patch_size=14, image_size=28,
                          projection_dim=1024, hidden_act="gelu", layer_norm_eps=1e-5)


@pytest.fixture(scope="module")
def tiny_clip(L):
    from tc_light_amd import clip
    sd = clip.seeded_state_dict(5, **TINY)
    frames = torch.randint(0, 256, (3, 30, 40, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    return sd, frames


def test_image_tokens_against_float64(L):
    """ip_adapter.image_tokens (one tcl_gemm_f16 at M = 2, one tcl_layernorm_f16 over [8, 768]) against tests/ip_refs.tokens_reference on the same
    f16-valued operands, every element inside tokens_bound; entry 0 is the zero embedding's tokens whatever the image."""
    from tc_light_amd import ip_adapter as IP
    proj, _ = IP.check_state(IP.seeded_state_dict(3))
    proj16 = {k: v.half().float() for k, v in proj.items()}
    g = torch.Generator().manual_seed(23)
    emb = torch.randn(1024, generator=g).half().float()
    got = IP.image_tokens(emb, proj, "cuda")
    zero = IP.image_tokens(torch.zeros(1024), proj, "cuda")
    other = IP.image_tokens(torch.randn(1024, generator=g), proj, "cuda")
    torch.cuda.synchronize()
    assert got.shape == (2, 4, 768) and got.dtype == torch.float16 and got.is_contiguous()
    ref, bound = R.tokens_reference(emb, proj16), R.tokens_bound(emb, proj16)
    err = (got.double().cpu() - ref).abs()
    print(f"image tokens: max |err| {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}, |cond - uncond| max "
          f"{(ref[1] - ref[0]).abs().max().item():.2f}")
    assert torch.isfinite(got.float()).all() and (err <= bound).all()
    assert (bound < 0.05).all() and (ref[1] - ref[0]).abs().max().item() > 0.5      # the bound cannot hide a swapped or wrong entry
    bits = lambda t: t.cpu().view(torch.int16)
    assert torch.equal(bits(zero[0]), bits(zero[1])) and torch.equal(bits(got[0]), bits(zero[0])) and torch.equal(bits(other[0]), bits(got[0]))
    assert not torch.equal(bits(other[1]), bits(got[1]))


def test_vision_engine_equals_the_full_engine(tiny_clip):
    """CLIPVisionEngine on the visual.* tensors alone gives the bits CLIPEngine gives on the whole state, and holds no text tower."""
    from tc_light_amd import clip
    sd, frames = tiny_clip
    full = clip.CLIPEngine(sd, "cuda", text_heads=1, **TINY_KW)
    vis = clip.CLIPVisionEngine(clip.visual_state(sd), "cuda", **TINY_KW)
    a, b = full.encode_image(frames, batch=2), vis.encode_image(frames, batch=2)
    torch.cuda.synchronize()
    assert a.shape == (3, 1024) and torch.isfinite(a).all() and torch.equal(a, b)
    assert (a[0] - a[1]).abs().max().item() > 1e-3              # the features depend on the image
    assert not hasattr(vis, "ttower") and not hasattr(vis, "encode_text") and isinstance(full, clip._ImageTower)
    via = clip.vision_engine(clip.visual_state(sd), "cuda", TINY_VISION_CONFIG)
    assert torch.equal(via.encode_image(frames), a)
    with pytest.raises(KeyError, match="visual.proj"):
        clip.CLIPVisionEngine({k: v for k, v in sd.items() if k != "visual.proj"}, "cuda", **TINY_KW)


def _save_snapshot(path, tensors, config):
    import json
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    save_file({k: v.contiguous().clone() for k, v in tensors.items()}, os.path.join(path, "model.safetensors"))
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(config, f)


def test_image_encoder_snapshots_load(tiny_clip, tmp_path):
    """models.image_encoder as a CLIPVisionModelWithProjection snapshot, as one file, and as a CLIPModel snapshot (PickScore's layout): the same
    visual.* tensors, and an engine built from each gives the same bits."""
    from tc_light_amd import clip
    from tc_light_amd.model_utils import load_image_encoder_state
    sd, frames = tiny_clip
    hf = clip.to_hf_state(sd)
    vision_only = {k: v for k, v in hf.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
    _save_snapshot(str(tmp_path / "vision"), vision_only, TINY_VISION_CONFIG)
    _save_snapshot(str(tmp_path / "whole"), hf, clip.to_hf_config(dict(TINY, vision_heads=1, text_heads=1, act="gelu")))
    want = clip.visual_state(sd)
    ref = clip.CLIPVisionEngine(want, "cuda", **TINY_KW).encode_image(frames)
    for path in (str(tmp_path / "vision"), str(tmp_path / "vision" / "model.safetensors"), str(tmp_path / "whole")):
        state, config = load_image_encoder_state(path)
        assert set(state) == set(want) and all(torch.equal(state[k], want[k]) for k in want), path
        assert (config is None) == path.endswith(".safetensors")
        eng = clip.vision_engine(state, "cuda", config if config is not None else TINY_VISION_CONFIG)
        assert torch.equal(eng.encode_image(frames), ref), path
    with pytest.raises(FileNotFoundError, match="image encoder"):
        load_image_encoder_state(str(tmp_path / "nowhere"))
    os.makedirs(tmp_path / "empty")
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        load_image_encoder_state(str(tmp_path / "empty"))


def test_build_end_to_end(tiny_clip, tmp_path):
    """ip_adapter.build, the one path run.py --ip_image takes: a PNG on disk, an image encoder snapshot on disk (toy size, ViT-H/14's interface), the
    adapter's seeded stand-in -> an ImagePrompt whose tokens are image_tokens(encode_image(the PNG)) bit for bit; the encoder is gone afterwards."""
    import numpy as np
    from PIL import Image
    from tc_light_amd import clip
    from tc_light_amd import ip_adapter as IP
    from tc_light_amd.unet import ImagePrompt
    sd, _ = tiny_clip
    hf = clip.to_hf_state(sd)
    _save_snapshot(str(tmp_path / "enc"), {k: v for k, v in hf.items() if k.startswith("vision_model.") or k == "visual_projection.weight"},
                   TINY_VISION_CONFIG)
    img = np.random.default_rng(4).integers(0, 256, (37, 50, 3), dtype=np.uint8)
    Image.fromarray(img).save(str(tmp_path / "ref.png"))
    block = dict(image=str(tmp_path / "ref.png"), scale=0.7, path=None, image_encoder=str(tmp_path / "enc"))
    u8 = IP.read_image_u8(block["image"])
    assert u8.shape == (1, 37, 50, 3) and u8.dtype == torch.uint8 and np.array_equal(u8[0].numpy(), img)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    with pytest.warns(UserWarning, match="IP-Adapter"):         # the adapter file is the seeded stand-in: allow=True, and it says so
        ip = IP.build(block, "cuda", allow=True)
    torch.cuda.synchronize()
    held = ip.tokens.numel() * 2 + sum(w.numel() * 2 for w in ip.weights.values())
    after = torch.cuda.memory_allocated()
    print(f"build: the ImagePrompt holds {held / 2 ** 20:.1f} MiB, allocated grew by {(after - before) / 2 ** 20:.1f} MiB")
    assert isinstance(ip, ImagePrompt) and ip.tokens.shape == (2, 4, 768) and ip.tokens.dtype == torch.float16 and ip.scale == 0.7 and ip.n_tokens == 4
    assert set(ip.weights) == set(IP.BLOCK_OF_INDEX.values()) and all(w.is_cuda and w.dtype == torch.float16 for w in ip.weights.values())
    assert after - before <= held + (1 << 20)                    # nothing of the encoder is still allocated (1 MiB: allocation rounding)
    proj, weights = IP.check_state(IP.seeded_state_dict(10))
    emb = clip.CLIPVisionEngine(clip.visual_state(sd), "cuda", **TINY_KW).encode_image(u8)[0]
    want = IP.image_tokens(emb, proj, "cuda")
    assert torch.equal(ip.tokens.view(torch.int16), want.view(torch.int16))
    assert torch.equal(ip.weights["mid_block.attentions.0."].cpu(), weights["mid_block.attentions.0."].half())
    with pytest.raises(FileNotFoundError, match="IP-Adapter"):   # without allow the missing adapter file is an error, as for every other model
        IP.build(block, "cuda")
