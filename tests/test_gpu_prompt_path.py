"""GPU: generation.prompt_path, a text conditioning per frame (tcl_text_lerp_f16 in csrc/text_lerp.hip, tcl_attention_kvindex_f16 in csrc/attn.hip,
unet.FrameText, Generator.frame_text).
  * the blend kernel against the host restatement of its float sequence (tests/prompt_refs.py), bit for bit; t = 0 / 1 copy the keyframe's bits;
  * the attention with a K / V entry per sample: every sample equals, bit for bit, the same kernel run on that sample alone with its entry handed
    over through kv_div; a null table is tcl_attention_f16; an entry out of range is TCL_EINVAL and nothing is launched;
  * a UNet pass with per-frame text whose rows are all E is the single-text pass with E, bit for bit; two distinct rows change it, swapping them
    changes it again, and renumbering the rows without changing any frame's text changes nothing;
  * run.py --prompt_sweep A A is the -p A run bit for bit, --prompt_sweep A B is not.
Seeded random weights everywhere: parity and plumbing, not image quality."""
import os
import sys

import numpy as np
import pytest
import torch

import prompt_refs as PR

pytestmark = pytest.mark.gpu
H16 = torch.float16
EINVAL = "TCL_EINVAL"
PACK_KV, PAIR, PREPACKED = 1, 2, 4


@pytest.fixture(scope="module", autouse=True)
def _leave_no_garbage():
    yield
    import gc
    gc.collect()


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- the blend, bit for bit
def _lerp(L, keys, rows, guard=16, offset=0):
    """One launch over len(rows) frames -> ([F, LD] f16 numpy, the guard halves behind it).  offset: halves by which out and keys are moved off a
    16 B boundary (the element-by-element path)."""
    K, LD = keys.shape
    F = len(rows)
    kbuf = torch.zeros(K * LD + 8, dtype=H16, device="cuda")
    kbuf[offset:offset + K * LD] = torch.from_numpy(keys.reshape(-1)).cuda()
    out = torch.full((F * LD + guard + 8,), -7.0, dtype=H16, device="cuda")
    tab = torch.tensor([[k0, k1, PR.t_bits(t)] for k0, k1, t in rows], dtype=torch.int32)
    L.tcl_text_lerp_f16(out[offset:], kbuf[offset:], K, tab.cuda(), tab, F, LD, st())
    got = out.cpu().numpy()
    return got[offset:offset + F * LD].reshape(F, LD), np.concatenate([got[:offset], got[offset + F * LD:]])


def test_text_lerp_bits(L):
    Lt, D = 77, 768
    keys = PR.make_keys(3, Lt, D, seed=1)
    rows = [(0, 1, 0.0), (0, 1, 1.0), (0, 1, 0.5), (0, 1, 1.0 / 3.0), (2, 0, 1.0 / 3.0)]         # F = 5, t from {0, 1, 0.5, 1/3}
    want = PR.lerp_rows(keys, rows)
    got, guard = _lerp(L, keys, rows)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert np.array_equal(got[0].view(np.uint16), keys[0].view(np.uint16))                     # t = 0: the bits of keyframe k0 (-0 stays -0)
    assert np.array_equal(got[1].view(np.uint16), keys[1].view(np.uint16))                     # t = 1: the bits of keyframe k1
    assert (guard == -7.0).all()
    sub = (np.abs(want[2:].astype(np.float32)) < 2.0 ** -14) & (want[2:] != 0)
    assert sub.any() and np.isfinite(want.astype(np.float32)).all()                            # blended rows do produce f16 subnormals


def test_text_lerp_scalar_path_and_odd_length(L):
    """LD = 3 * 37 = 111 (no multiple of 8) and a buffer 2 B off a 16 B boundary: the element-by-element path, same sequence."""
    keys = PR.make_keys(3, 3, 37, seed=2)
    rows = [(1, 2, 1.0 / 3.0), (2, 2, 0.0), (0, 2, 1.0), (1, 0, 0.5)]
    want = PR.lerp_rows(keys, rows)
    got, guard = _lerp(L, keys, rows)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)) and (guard == -7.0).all()
    keys8, rows8 = PR.make_keys(2, 2, 64, seed=3), [(0, 1, 1.0 / 3.0), (1, 0, 0.0)]
    got8, guard8 = _lerp(L, keys8, rows8, offset=1)                  # LD = 128, but both bases 2 B off
    assert np.array_equal(got8.view(np.uint16), PR.lerp_rows(keys8, rows8).view(np.uint16)) and (guard8 == -7.0).all()


def test_text_lerp_refuses(L):
    keys = torch.zeros(2, 64, dtype=H16, device="cuda")
    out = torch.full((2, 64), -7.0, dtype=H16, device="cuda")

    def call(rows, n_keys=2, F=None, LD=64, h_tab=True):
        tab = torch.tensor([[k0, k1, PR.t_bits(t)] for k0, k1, t in rows], dtype=torch.int32)
        L.tcl_text_lerp_f16(out, keys, n_keys, tab.cuda(), tab if h_tab else 0, len(rows) if F is None else F, LD, st())
    for rows in ([(0, 2, 0.5), (0, 1, 0.5)], [(0, 1, 0.5), (-1, 1, 0.5)], [(0, 1, 1.5)], [(0, 1, -0.25)], [(0, 1, float("nan"))]):
        with pytest.raises(RuntimeError, match=EINVAL):
            call(rows)
    for kw in (dict(n_keys=0), dict(F=0), dict(LD=0), dict(h_tab=False)):
        with pytest.raises(RuntimeError, match=EINVAL):
            call([(0, 1, 0.5)], **kw)
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                      # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- attention with a K / V entry per sample
def _attn_inputs(B, H, Tq, Lt, d, rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, Tq, H * d, device="cuda", generator=g).half()
    k = torch.randn(rows, Lt, H * d, device="cuda", generator=g).half()
    v = torch.randn(rows, Lt, H * d, device="cuda", generator=g).half()
    return q, k, v


def _ws(L, B, Bkv, H, Tq, Lt, d):
    return (torch.empty(L.tcl_attention_q_bytes(B, H, Tq, d), dtype=torch.uint8, device="cuda"),
            torch.empty(L.tcl_attention_kv_bytes(Bkv, H, Lt, d), dtype=torch.uint8, device="cuda"))


def _plain(L, q, k, v, H, d, kv_div):
    """tcl_attention_f16 on q [B,Tq,Hd] against k / v [B / kv_div, Lt, Hd]."""
    B, Tq, C = q.shape
    Lt = k.shape[1]
    o = torch.full((B, Tq, C), -7.0, dtype=H16, device="cuda")
    wq, wkv = _ws(L, B, B // kv_div, H, Tq, Lt, d)
    L.tcl_attention_f16(q, C, Tq * C, k, C, Lt * C, v, C, Lt * C, o, C, Tq * C, B, H, Tq, Lt, d, d ** -0.5, kv_div, PACK_KV, wq, wkv, st())
    return o


def _indexed(L, q, k, v, H, d, index, flags=PACK_KV, ws=None, kv_div=1):
    B, Tq, C = q.shape
    rows, Lt = k.shape[0], k.shape[1]
    o = torch.full((B, Tq, C), -7.0, dtype=H16, device="cuda")
    wq, wkv = ws if ws is not None else _ws(L, B, rows, H, Tq, Lt, d)
    host = torch.tensor(index, dtype=torch.int32)
    L.tcl_attention_kvindex_f16(q, C, Tq * C, k, C, Lt * C, v, C, Lt * C, o, C, Tq * C, B, H, Tq, Lt, d, d ** -0.5, kv_div, flags, wq, wkv,
                                host.cuda(), host, rows, st())
    return o, (wq, wkv)


INDEX = [2, 0, 2, 1, 1, 0]                                          # repeats, not monotone, every row used


@pytest.mark.parametrize("d", [40, 160])
@pytest.mark.parametrize("Tq", [64, 70])
def test_indexed_attention_equals_each_sample_alone(L, d, Tq):
    B, H, Lt, rows = 6, 8, 77, 3
    q, k, v = _attn_inputs(B, H, Tq, Lt, d, rows, seed=d + Tq)
    got, ws = _indexed(L, q, k, v, H, d, INDEX)
    for b in range(B):
        r = INDEX[b]
        alone = _plain(L, q[b:b + 1].contiguous(), k[r:r + 1].contiguous(), v[r:r + 1].contiguous(), H, d, 1)
        assert torch.equal(got[b], alone[0]), (b, r)
    assert torch.isfinite(got.float()).all() and got.float().std() > 0
    # the panels packed once serve another table (what the UNet does from the second pass on): Q packed from the tensor, K / V as they lie in ws_kv
    other = [0, 1, 1, 2, 0, 2]
    again, _ = _indexed(L, q, k, v, H, d, other, flags=0, ws=ws)
    for b in range(B):
        r = other[b]
        alone = _plain(L, q[b:b + 1].contiguous(), k[r:r + 1].contiguous(), v[r:r + 1].contiguous(), H, d, 1)
        assert torch.equal(again[b], alone[0]), (b, r)


def test_indexed_attention_large_grid_d40(L):
    """B H ceil256(Tq) / 256 >= 1024 blocks: head_dim 40 takes the speculative two-query-block kernel and its gated exact pass, the variant a level-0
    pass runs.  The variant is chosen from B, so the reference is the same B through the existing path: K / V gathered to one entry per sample,
    kv_div = 1.  Tq = 5500 is no multiple of the 256-query block."""
    B, H, Tq, Lt, d, rows = 6, 8, 5500, 77, 40, 3
    plan = np.zeros(4, dtype=np.int32)
    L.tcl_attention_plan(B, H, Tq, Lt, d, 1, PACK_KV, plan.ctypes.data)
    assert plan[0] == 0 and plan[2] > 0                             # the speculative kernel, with a gated pass behind it
    q, k, v = _attn_inputs(B, H, Tq, Lt, d, rows, seed=5)
    got, _ = _indexed(L, q, k, v, H, d, INDEX)
    idx = torch.tensor(INDEX, device="cuda")
    want = _plain(L, q, k[idx].contiguous(), v[idx].contiguous(), H, d, 1)
    assert torch.equal(got, want) and torch.isfinite(got.float()).all()


@pytest.mark.parametrize("d", [40, 160])
def test_null_table_is_the_existing_call(L, d):
    B, H, Tq, Lt = 6, 8, 70, 77
    q, k, v = _attn_inputs(B, H, Tq, Lt, d, 2, seed=d)
    want = _plain(L, q, k, v, H, d, 3)                              # the text cross-attention's mapping: b // (B / 2)
    C = H * d
    o = torch.full((B, Tq, C), -7.0, dtype=H16, device="cuda")
    wq, wkv = _ws(L, B, 2, H, Tq, Lt, d)
    L.tcl_attention_kvindex_f16(q, C, Tq * C, k, C, Lt * C, v, C, Lt * C, o, C, Tq * C, B, H, Tq, Lt, d, d ** -0.5, 3, PACK_KV, wq, wkv, 0, 0, 0, st())
    assert torch.equal(o, want)
    got, _ = _indexed(L, q, k, v, H, d, [0, 0, 0, 1, 1, 1])          # and the table that spells that mapping out
    assert torch.equal(got, want)


@pytest.mark.parametrize("bad", [[2, 0, 3, 1, 1, 0], [2, 0, 2, 1, -1, 0]])
def test_index_out_of_range_is_refused_without_a_launch(L, bad):
    B, H, Tq, Lt, d = 6, 8, 64, 77, 40
    q, k, v = _attn_inputs(B, H, Tq, Lt, d, 3, seed=9)
    C = H * d
    o = torch.full((B, Tq, C), -7.0, dtype=H16, device="cuda")
    wq, wkv = _ws(L, B, 3, H, Tq, Lt, d)
    wq.fill_(0x5A)
    wkv.fill_(0x5A)
    host = torch.tensor(bad, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=EINVAL):
        L.tcl_attention_kvindex_f16(q, C, Tq * C, k, C, Lt * C, v, C, Lt * C, o, C, Tq * C, B, H, Tq, Lt, d, d ** -0.5, 1, PACK_KV, wq, wkv,
                                    host.cuda(), host, 3, st())
    with pytest.raises(RuntimeError, match=EINVAL):                 # a device table without its host copy cannot be checked: refused too
        L.tcl_attention_kvindex_f16(q, C, Tq * C, k, C, Lt * C, v, C, Lt * C, o, C, Tq * C, B, H, Tq, Lt, d, d ** -0.5, 1, PACK_KV, wq, wkv,
                                    host.cuda(), 0, 3, st())
    torch.cuda.synchronize()
    assert (o == -7.0).all() and (wq == 0x5A).all() and (wkv == 0x5A).all()       # neither the pack nor the attention ran


# ---------------------------------------------------------------------------------------------------------------- the UNet with per-frame text
HH, WW, T_STEP = 16, 24, 601.0
FS, FRAMES = [2, 2], [2, 3, 0, 1]                                   # xy mode, two chunks; the pass draws the frames out of clip order
DRAWS = [(1, 0.9), (0, 0.2)]


@pytest.fixture(scope="module")
def unet(L):
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    tome = VidToMe("cuda", seed=5)
    eng = UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(), seed=1), "cuda", tome)
    g = torch.Generator(device="cuda").manual_seed(21)
    xh = torch.randn(sum(FS), HH, WW, 8, device="cuda", generator=g).half()
    emb = torch.randn(3, 77, 768, device="cuda", generator=g).half()     # the negative, E and another prompt
    return eng, tome, torch.cat([xh, xh]).contiguous(), emb


def _passes(unet, text, frames=None):
    """Two passes (the second meets packed text K / V and takes the fused query-panel route) from fresh banks and the same draws."""
    eng, tome, x, _ = unet
    tome.reset_global_tokens()
    outs = []
    for _ in range(2):
        tome.draws = list(DRAWS)
        kw = {} if frames is None else dict(frames=frames)
        outs.append(eng.forward_many(x, FS, HH, WW, T_STEP, text, cfg_pair=True, **kw).clone())
    tome.reset_global_tokens()
    tome.draws = None
    torch.cuda.synchronize()
    return outs


@pytest.fixture(scope="module")
def single(unet):
    """The existing single-text pass with (negative, E): computed once, shared and left unchanged."""
    emb = unet[3]
    return _passes(unet, emb[:2].contiguous())


def test_constant_path_equals_single_prompt(unet, single):
    from tc_light_amd.unet import FrameText
    emb = unet[3]
    ft = FrameText(emb[0], torch.stack([emb[1], emb[1]]), [0, 1, 1, 0])          # two rows, both E: every frame's text is E
    got = _passes(unet, ft, FRAMES)
    for a, b in zip(got, single):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    one = _passes(unet, FrameText(emb[0], emb[1:2], [0, 0, 0, 0]), FRAMES)       # ... and one shared row
    for a, b in zip(one, single):
        assert torch.equal(a, b)


def test_frames_really_differ(unet, single):
    from tc_light_amd.unet import FrameText
    emb = unet[3]
    rows = torch.stack([emb[1], emb[2]])
    index = [0, 0, 1, 1]                                           # frames 0, 1 read E, frames 2, 3 the other prompt
    two = _passes(unet, FrameText(emb[0], rows, index), FRAMES)
    Ft = sum(FS)
    for a, b in zip(two, single):
        assert not torch.equal(a, b)
        cond_a, cond_b = a.view(2 * Ft, -1)[Ft:], b.view(2 * Ft, -1)[Ft:]
        # the samples of frames 2, 3 (first chunk) changed; the unconditional half shares the negative and, in the level-0 blocks, the merged tokens
        assert not torch.equal(cond_a[0], cond_b[0]) and not torch.equal(cond_a[1], cond_b[1])
    swapped = _passes(unet, FrameText(emb[0], rows, [1, 1, 0, 0]), FRAMES)
    for a, b in zip(swapped, two):
        assert not torch.equal(a, b)
    # the rows renumbered and the table with them: every frame keeps its text, so nothing changes
    renum = _passes(unet, FrameText(emb[0], torch.stack([emb[2], emb[1]]), [1, 1, 0, 0]), FRAMES)
    for a, b in zip(renum, two):
        assert torch.equal(a, b)
    # a third row nobody reads changes nothing either
    spare = _passes(unet, FrameText(emb[0], torch.stack([emb[0], emb[2], emb[1]]), [2, 2, 1, 1]), FRAMES)
    for a, b in zip(spare, two):
        assert torch.equal(a, b)


def test_forward_many_wants_the_frames_of_a_per_frame_text(unet):
    from tc_light_amd.unet import FrameText
    eng, _, x, emb = unet
    ft = FrameText(emb[0], emb[1:3].contiguous(), [0, 1, 1, 0])
    with pytest.raises(ValueError, match="frames"):
        eng.forward_many(x, FS, HH, WW, T_STEP, ft, cfg_pair=True)
    with pytest.raises(ValueError, match="frames"):
        eng.forward_many(x, FS, HH, WW, T_STEP, ft, cfg_pair=True, frames=[0, 1])
    with pytest.raises(ValueError):
        FrameText(emb[0], emb[1:3].contiguous(), [0, 2])
    assert eng.text_rows_bytes(3) == sum(eng.L.tcl_attention_kv_bytes(3, 8, 77, c // 8) for c in [320] * 5 + [640] * 5 + [1280] * 6)


def test_frame_text_blends_the_rows_of_the_ranks_frames(L, unet):
    """Generator.frame_text: one row per distinct (k0, k1, t) of the rank's frames, each the host sequence's bits; rank 1 of 2 holds its own rows."""
    from types import SimpleNamespace
    from tc_light_amd.generate import Generator
    from tc_light_amd.parallel import Dist
    emb = unet[3]
    A, B = "sunrise", "dusk"
    stub = SimpleNamespace(dev=torch.device("cuda"), tome=SimpleNamespace(args={}))
    keys = emb[1:3].contiguous()
    knp = keys.cpu().numpy().reshape(2, -1)
    g = Generator(stub, None, dict(prompt_path=[[0, A], [1, B]], max_tokens_per_pass=1 << 20))
    ft = g.frame_text(emb[0], keys, 5)
    assert ft.index == [0, 1, 2, 3, 4] and g.prompt_rows == [(0, 0, 0.0), (0, 1, 0.25), (0, 1, 0.5), (0, 1, 0.75), (1, 1, 0.0)]
    want = PR.lerp_rows(knp, g.prompt_rows)
    assert torch.equal(ft.text[0], emb[0])
    assert np.array_equal(ft.text[1:].cpu().numpy().reshape(5, -1).view(np.uint16), want.view(np.uint16))
    g1 = Generator(stub, None, dict(prompt_path=[[0, A], [1, B]], max_tokens_per_pass=1 << 20), dist=Dist(1, 2))
    ft1 = g1.frame_text(emb[0], keys, 2, n_total=5)
    assert ft1.index == [0, 1] and g1.prompt_rows == [(0, 1, 0.75), (1, 1, 0.0)]
    assert torch.equal(ft1.text[1:], ft.text[4:])


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_prompt_sweep(L, tmp_path):
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(__file__))
    import synth
    import run
    d = synth.video_clip(3, 64, 64, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    A, B = "warm light from the left", "cold moonlight, deep blue shadows"

    def go(tag, *args):
        work = tmp_path / tag
        cfg = tmp_path / f"{tag}.yaml"
        cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {work}
data: {{rgb_path: {vid}, height: 64, width: 64}}
generation:
  prompt: {{edit: "{A}"}}
  n_timesteps: 2
  alpha_t: 0.01
  frame_range: [0, 3, 1]
post_opt: {{apply_opt: false}}
models: {{allow_random: true}}
""")
        cwd = os.getcwd()
        os.chdir(tmp_path)
        try:
            run.main(["--config", str(cfg), *args])
        finally:
            os.chdir(cwd)
        outs = [os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs if f == "output.npy"]
        assert len(outs) == 1
        return np.load(outs[0]), outs[0]
    plain, _ = go("plain", "-p", A)
    same, path = go("same", "--prompt_sweep", A, A)
    assert plain.shape == (3, 64, 64, 3) and plain.dtype == np.uint8 and plain.std() > 0
    assert np.array_equal(same, plain)
    import yaml
    gs = yaml.safe_load(open(os.path.join(os.path.dirname(path), "config.yaml")))["generation"]
    assert gs["prompt_path"] == [[0.0, A], [1.0, A]] and gs["prompt"] == {"edit": A}
    other, _ = go("other", "--prompt_sweep", A, B)
    assert other.shape == plain.shape and not np.array_equal(other, plain)
    assert not np.array_equal(other[2], plain[2])                   # the last frame is conditioned on B alone
