"""GPU: the background-conditioned IC-Light model (generation.iclight_model: fbc; utils/model_utils.py:97-179 init_iclight_bg).
  * tcl_pack_latents12_f16 bit for bit against torch indexing (tests/fbc_refs.py): xy and yt, one background latent and one per frame, the output
    inside a NaN-filled buffer at a 16 B and at an 8 B aligned offset, both CFG halves, the refusals;
  * tcl_matte_grey_f32 and tcl_bg_ramp_f32: the stored integers exactly, at 5x7 (scalar path) and 64x64 (16 B path);
  * a 12-channel UNetEngine.forward_many against oracle.sd15.unet_forward, and channels 8-11 are live;
  * test_ddim_sample_multi_axis_vs_oracle restated with the 8-channel condition, one background frame and one per frame;
  * the Generator and run.py end to end.
Seeded random weights everywhere: parity and plumbing, not image quality."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import fbc_refs as R

pytestmark = pytest.mark.gpu
H16 = torch.float16


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


@pytest.fixture(scope="module")
def sd12(L):
    from tc_light_amd import sd15
    return sd15.random_state_dict(sd15.unet_param_shapes(in_channels=12), seed=1)


@pytest.fixture(scope="module")
def eng(sd12):
    """The 12-channel engine with VidToMe off: no discrete choices in the comparisons with the oracle."""
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    return UNetEngine(sd12, "cuda", VidToMe("cuda", seed=5, enabled=False))


@pytest.fixture(scope="module")
def unet(sd12):
    """The same weights with VidToMe on, for the end-to-end runs (every run installs a fresh VidToMe)."""
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    return UNetEngine(sd12, "cuda", VidToMe("cuda", seed=5))


@pytest.fixture(scope="module")
def vae(L):
    from tc_light_amd import sd15
    from tc_light_amd.vae import VAEEngine
    return VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")


@pytest.fixture(scope="module")
def rmbg(L):
    from tc_light_amd.model_utils import load_rmbg_state
    from tc_light_amd.rmbg import RMBGEngine
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return RMBGEngine(load_rmbg_state(None, allow=True), "cuda")


def st():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


# ---------------------------------------------------------------------------------------------------------------- the pack kernel, bit for bit
def _latents(N=5, h=3, w=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(N, 4, h, w, generator=g).to(H16) for _ in range(3))


@pytest.mark.parametrize("guard", [16, 4], ids=["out16B", "out8B"])        # halves in front of `out`: both orders of the 16 B + 8 B stores
@pytest.mark.parametrize("bg_frames", [1, 5])
@pytest.mark.parametrize("mode", ["xy", "yt"])
def test_pack_latents12_bits(L, mode, bg_frames, guard):
    N, h, w = 5, 3, 5
    x, fg, bg = _latents(N, h, w)
    bg = bg[:bg_frames].contiguous()
    if mode == "xy":
        idx, args, shape = [4, 0, 4], (0, 0, 0), (6, h, w, 12)
    else:
        idx, args, shape = [3, 0], (1, 1, 3), (4, 3, h, 12)
    want = R.pack12(x, fg, bg, idx, *args)
    assert tuple(want.shape) == shape
    numel = want.numel()
    buf = torch.full((guard + numel + 24,), float("nan"), dtype=H16, device="cuda")
    out = buf[guard:guard + numel]
    L.tcl_pack_latents12_f16(x.cuda(), fg.cuda(), bg.cuda(), bg_frames, torch.tensor(idx, dtype=torch.int32, device="cuda"), len(idx), *args, h, w,
                             out, st())
    got = buf.cpu()
    assert torch.isnan(got[:guard]).all() and torch.isnan(got[guard + numel:]).all()               # the guards survive
    got = got[guard:guard + numel].view(shape)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))                              # bit for bit
    F = len(idx)
    assert torch.equal(got[:F].view(torch.int16), got[F:].view(torch.int16))                        # both CFG halves


def test_pack_latents12_more_than_one_tile(L):
    """yt with more columns and rows than one 32 x 32 transposition tile, and xy over more than one block."""
    N, h, w = 3, 37, 41
    x, fg, bg = _latents(N, h, w, seed=8)
    cols = list(range(w - 1, -1, -1))[:35] + [0, 7]
    out = torch.empty(2 * len(cols), 2, h, 12, dtype=H16, device="cuda")
    L.tcl_pack_latents12_f16(x.cuda(), fg.cuda(), bg.cuda(), N, torch.tensor(cols, dtype=torch.int32, device="cuda"), len(cols), 1, 1, 2, h, w, out, st())
    assert torch.equal(out.cpu().view(torch.int16), R.pack12(x, fg, bg, cols, 1, 1, 2).view(torch.int16))
    out = torch.empty(4, h, w, 12, dtype=H16, device="cuda")
    L.tcl_pack_latents12_f16(x.cuda(), fg.cuda(), bg[:1].cuda(), 1, torch.tensor([2, 1], dtype=torch.int32, device="cuda"), 2, 0, 0, 0, h, w, out, st())
    assert torch.equal(out.cpu().view(torch.int16), R.pack12(x, fg, bg[:1], [2, 1], 0).view(torch.int16))


def test_pack_latents12_refusals(L):
    N, h, w = 5, 3, 5
    x, fg, bg = (t.cuda() for t in _latents(N, h, w))
    idx = torch.tensor([4, 0, 4], dtype=torch.int32, device="cuda")
    out = torch.zeros(6 * h * w * 12 + 8, dtype=H16, device="cuda")
    good = [x, fg, bg, N, idx, 3, 0, 0, 0, h, w, out]
    L.tcl_pack_latents12_f16(*good, st())
    for pos in (0, 1, 2, 4, 11):                                           # null pointers
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_pack_latents12_f16(*[0 if k == pos else v for k, v in enumerate(good)], st())
    for pos, bad in ((5, 0), (5, -2), (3, 0), (3, -1), (6, 2), (9, 0), (10, 0)):      # F <= 0, bg_frames < 1, another mode, empty planes
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_pack_latents12_f16(*[bad if k == pos else v for k, v in enumerate(good)], st())
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):                  # an output that is not 8 B aligned
        L.tcl_pack_latents12_f16(*good[:11], out[1:], st())
    # yt: frames sl .. sl + nwin = 1 .. 4 are read, so a per-frame background of 2 or 3 frames is neither 1 nor N
    for bad in (2, 3):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_pack_latents12_f16(x, fg, bg, bad, idx, 2, 1, 1, 3, h, w, out, st())
    for sl, nwin in ((-1, 3), (1, 0)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_pack_latents12_f16(x, fg, bg, N, idx, 2, 1, sl, nwin, h, w, out, st())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- ramp and matte, exact integers
@pytest.mark.parametrize("H,W", [(5, 7), (64, 64)])
def test_bg_ramp_integers(L, H, W):
    from tc_light_amd import hostlogic as HL
    for source in ("left", "right", "top", "bottom", "grey"):
        side, start, stop = HL.BG_RAMPS[source]
        buf = torch.full((3 * H * W + 4,), float("nan"), device="cuda")
        L.tcl_bg_ramp_f32(buf, H, W, side, start, stop, st())
        got = buf.cpu().numpy()
        assert np.isnan(got[3 * H * W:]).all()
        got = got[:3 * H * W].reshape(3, H, W)
        u = R.ramp_u8(source, H, W)
        want = np.broadcast_to(u.astype(np.float32) / np.float32(254), (3, H, W))                  # one IEEE division
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), source
        assert np.array_equal(np.rint(np.float32(254) * got).astype(np.int64), np.broadcast_to(u.astype(np.int64), (3, H, W))), source
    out = torch.empty(3, H, W, device="cuda")
    for args in ((0, H, W, 0, 224, 32), (out, 0, W, 0, 224, 32), (out, H, W, 4, 224, 32), (out, H, W, 0, 256, 32), (out, H, W, 0, 224, -1)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_bg_ramp_f32(*args, st())


@pytest.mark.parametrize("H,W", [(5, 7), (64, 64)])
def test_matte_grey_integers(L, H, W):
    n = 2
    rng = np.random.default_rng(H * 100 + W)
    f = rng.random((n, 3, H, W), dtype=np.float32)
    a = rng.random((n, 1, H, W), dtype=np.float32)
    us = np.array([0, 126, 127, 128, 255], dtype=np.float32) / np.float32(255)
    f.reshape(-1)[:15] = np.repeat(us, 3)                                   # the table of the reference's own test, at the three alphas
    f.reshape(-1)[15:18] = [-0.5, 1.5, 1.0]                                 # outside [0, 1]: the clamp
    a[0, 0].reshape(-1)[:18] = np.tile(np.array([0.0, 0.5, 1.0], dtype=np.float32), 6)
    a[1, 0, -1, -3:] = [0.0, 1.0, 0.5]
    buf = torch.full((n * 3 * H * W + 4,), float("nan"), device="cuda")
    L.tcl_matte_grey_f32(torch.from_numpy(f).cuda(), torch.from_numpy(a).cuda(), buf, n, H, W, st())
    got = buf.cpu().numpy()
    assert np.isnan(got[n * 3 * H * W:]).all()
    got = got[:n * 3 * H * W].reshape(n, 3, H, W)
    q = R.matte_q(f, a)
    assert q.shape == (n, 3, H, W) and len(np.unique(q)) > 16
    want = q.astype(np.float32) / np.float32(254)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.rint(np.float32(254) * got).astype(np.int64), q)
    fd, ad, od = torch.from_numpy(f).cuda(), torch.from_numpy(a).cuda(), torch.empty(n, 3, H, W, device="cuda")
    for args in ((0, ad, od, n, H, W), (fd, 0, od, n, H, W), (fd, ad, 0, n, H, W), (fd, ad, od, 0, H, W), (fd, ad, od, n, 0, W)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_matte_grey_f32(*args, st())


# ---------------------------------------------------------------------------------------------------------------- the 12-channel UNet
@pytest.mark.parametrize("Hh,Ww", [(8, 8), (3, 5)])
def test_unet12_forward_many_vs_oracle(sd12, eng, Hh, Ww):
    """rel-L2 <= 1e-2: the bound test_gpu_unet.py and test_gpu_denoise_loop.py use for this f16-engine vs f32-oracle comparison."""
    from oracle import sd15 as OS
    Fs = [2, 1]
    F = sum(Fs)
    rng = np.random.default_rng(50 + Hh)
    x = torch.from_numpy(rng.standard_normal((F, 12, Hh, Ww)).astype(np.float32)).half().float()
    text = torch.from_numpy(rng.standard_normal((2, 77, 768)).astype(np.float32)).half().float()

    def run(xx):
        xin = torch.cat([xx, xx]).permute(0, 2, 3, 1).contiguous().cuda().half()
        return eng.forward_many(xin, Fs, Hh, Ww, 501.0, text.cuda().half()).view(2 * F, Hh, Ww, 4).permute(0, 3, 1, 2).float().cpu()
    eps = run(x)
    off, refs = 0, []
    for f in Fs:
        with torch.no_grad():
            ref = OS.unet_forward(sd12, torch.cat([x[off:off + f], x[off:off + f]]), 501.0, text)
        got = torch.cat([eps[off:off + f], eps[F + off:F + off + f]])
        r = rel(got, ref)
        print(f"[unet12] {Hh}x{Ww} chunk of {f}: rel-L2 = {r:.3e}")
        assert r < 1e-2, (Hh, Ww, f, r)
        refs.append(ref)
        off += f
    # another background latent moves eps by more than that bound: channels 8-11 reach the stem
    x2 = x.clone()
    x2[:, 8:] = torch.from_numpy(rng.standard_normal((F, 4, Hh, Ww)).astype(np.float32)).half().float()
    moved = rel(run(x2), eps)
    print(f"[unet12] {Hh}x{Ww}: eps moved by rel-L2 {moved:.3e} under another background latent")
    assert moved > 1e-2


# ---------------------------------------------------------------------------------------------------------------- the multi-axis loop
@pytest.mark.parametrize("bg_frames", [1, 6], ids=["one_bg", "per_frame_bg"])
def test_ddim_sample_multi_axis_fbc_vs_oracle(sd12, eng, bg_frames):
    """test_gpu_denoise_loop.py::test_ddim_sample_multi_axis_vs_oracle with the 8-channel condition: the oracle is fed cat([fg, bg.expand(n)], 1);
    its per-step bounds (fused eps rel-L2 <= 1e-2, latents after the SDE step <= 2e-3)."""
    from oracle import pipeline as OP
    from oracle import sd15 as OS
    from oracle.scheduler import Scheduler as OSch
    from tc_light_amd import hostlogic as HL
    from tc_light_amd.generate import Generator

    n, hh, ww = 6, 8, 8
    cfg = dict(n_timesteps=2, alpha_t=0.3, final_factor_t=0.5, win_size_t=4, chunk_size=4, guidance_scale=2.0, seed=77, noise_mode="vanilla",
               iclight_model="fbc", bg_source="grey", fbc_matting=False)
    g = Generator(eng, None, cfg)
    g.prepare_data(torch.zeros(n, 3, 8 * hh, 8 * ww, device="cuda"))
    gen = torch.Generator().manual_seed(3)
    conds = torch.randn(2, 154, 768, generator=gen).half()
    conds_t = torch.randn(2, 77, 768, generator=gen).half()
    fg = torch.randn(n, 4, hh, ww, generator=gen).half()
    bg = torch.randn(bg_frames, 4, hh, ww, generator=gen).half()
    x0 = g.init_noise.clone()

    zs, seen = [], []
    step = g.scheduler.step

    def recording_step(eps, t, x, noise=None, **kw):
        zs.append(None if noise is None else noise.float().cpu())
        seen.append((x.float().cpu(), eps.float().cpu()))          # latents entering the step, fused noise prediction
        return step(eps, t, x, noise=noise, **kw)
    g.scheduler.step = recording_step
    x_hip = g.ddim_sample(x0.clone(), conds.cuda(), conds_t.cuda(), (fg.cuda(), bg.cuda())).float().cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(x_hip).all() and len(zs) == 2 and zs[-1] is None

    c = g.cfg
    osch = OSch(c.n_timesteps)
    assert osch.timesteps.tolist() == g.scheduler.timesteps.tolist()
    alphas = OP.alpha_schedule(c.alpha_t, c.final_factor_t, c.n_timesteps)
    xy_s = HL.ChunkSampler(c.seed, c.chunk_size, c.merge_global, c.chunk_ord)
    yt_s = HL.ChunkSampler(c.seed + 1, c.chunk_size, c.merge_global, c.chunk_ord)
    ccf = torch.cat([fg, bg.expand(n, -1, -1, -1)], 1).float()
    x, text, text_t = x0.float().cpu(), conds.float(), conds_t.float()

    def pred(xin, txt, t):
        with torch.no_grad():
            return OP.cfg(OS.unet_forward(sd12, torch.cat([xin, xin]), t, txt), c.guidance_scale)

    def fused_eps(xc, xy_chunks, yt_chunks, i, t):
        noises = torch.zeros_like(xc)
        for ch in xy_chunks:
            noises[ch] = pred(torch.cat([xc[ch], ccf[ch]], 1), text, float(t))
        return OP.temporal_denoise(xc, ccf, alphas[i], noises, c.win_size_t, [torch.as_tensor(ch) for ch in yt_chunks],
                                   lambda xt, ct, ch, sl: pred(torch.cat([xt, ct], 1), text_t, float(t)))[1]

    nxt = [seen[1][0], x_hip]
    for i, t in enumerate(osch.timesteps.tolist()):
        xy_chunks, yt_chunks = xy_s.get_chunks(n), yt_s.get_chunks(ww)
        r = rel(seen[i][1], fused_eps(seen[i][0], xy_chunks, yt_chunks, i, t))
        print(f"[fbc denoise loop parity] bg_frames {bg_frames} step {i}: fused eps rel-L2 = {r:.3e}")
        assert r < 1e-2, (i, r)
        z = zs[i] if zs[i] is not None else torch.zeros_like(x)
        r = rel(nxt[i], osch.step(seen[i][1], seen[i][0], z))
        print(f"[fbc denoise loop parity] bg_frames {bg_frames} step {i}: latents after the SDE step rel-L2 = {r:.3e}")
        assert r < 2e-3, (i, r)


def test_ddim_sample_refuses_malformed_conditions(eng):
    from tc_light_amd.generate import Generator
    g = Generator(eng, None, dict(n_timesteps=1, iclight_model="fbc", bg_source="grey", fbc_matting=False, noise_mode="vanilla"))
    g.prepare_data(torch.zeros(3, 3, 64, 64, device="cuda"))
    cd = torch.zeros(2, 77, 768, dtype=H16, device="cuda")
    z = lambda k: torch.zeros(k, 4, 8, 8, dtype=H16, device="cuda")
    for cc in (z(3), (z(3), z(2)), (z(2), z(1)), (z(3), z(1).float())):      # not a pair; a background that is neither 1 nor n; ...
        with pytest.raises(ValueError, match="fbc"):
            g.ddim_sample(g.init_noise.clone(), cd, cd, cc)


# ---------------------------------------------------------------------------------------------------------------- the whole Generator
def _run(unet, vae, rmbg, **over):
    from tc_light_amd.generate import Generator
    from tc_light_amd.vidtome import VidToMe
    unet.tome = VidToMe("cuda", seed=5)                               # fresh draws: every run sees the same random frames / coins
    cfg = dict(n_timesteps=1, alpha_t=0.0, chunk_size=4, seed=31, noise_mode="same", apply_opt=False, iclight_model="fbc")
    cfg.update(over)
    g = Generator(unet, vae, cfg, rmbg=rmbg)
    gen = torch.Generator().manual_seed(9)
    frames = torch.rand(2, 3, 64, 64, generator=gen).cuda()
    background = torch.rand(1, 3, 64, 64, generator=gen).cuda()
    conds = torch.randn(2, 77, 768, generator=gen).half().cuda()
    out, info = g(frames, conds, conds, None, None, None, background=background if cfg.get("bg_source", "upload").startswith("upload") else None)
    torch.cuda.synchronize()
    return g, out, info, frames, background


@pytest.mark.parametrize("bg_source", ["left", "upload"])
def test_generator_fbc(L, unet, vae, rmbg, bg_source):
    ga, a, ia, frames, background = _run(unet, vae, rmbg, bg_source=bg_source)
    gb, b, _, _, _ = _run(unet, vae, rmbg, bg_source=bg_source)
    assert tuple(a.shape) == (2, 3, 64, 64) and a.dtype == torch.float32 and torch.isfinite(a).all()
    assert torch.equal(a, b)                                           # two runs, the same bits
    assert ia["iclight_model"] == "fbc" and torch.equal(ga.frames, frames)      # stage 1 / 2 and output_gt see the source frames
    assert tuple(ga.bg_frames.shape) == (1, 3, 64, 64) and tuple(ga.fg_frames.shape) == (2, 3, 64, 64)
    if bg_source == "left":
        assert np.array_equal(np.rint(254 * ga.bg_frames[0].cpu().numpy()).astype(np.int64), np.broadcast_to(R.ramp_u8("left", 64, 64), (3, 64, 64)))
    else:
        assert torch.equal(ga.bg_frames, background)
    # the matte: the stored integers of the reference on this run's frames and alpha
    alpha = rmbg.estimate_alpha(frames, 2)
    q = R.matte_q(frames.cpu().numpy(), alpha.float().cpu().numpy())
    assert np.array_equal(np.rint(254 * ga.fg_frames.cpu().numpy()).astype(np.int64), q)
    # the background is a live condition of the whole run
    _, c, _, _, _ = _run(unet, vae, rmbg, bg_source="grey")
    assert not torch.equal(a, c)


def test_generator_fbc_flip_and_no_matting(L, unet, vae):
    """fbc_matting: false never touches the RMBG engine (none is given, and one that is given is not called); upload_flip mirrors the background."""
    def no_alpha(*a, **k):
        raise AssertionError("fbc_matting: false, but the RMBG engine was asked for an alpha")
    g, out, _, frames, background = _run(unet, vae, None, bg_source="upload_flip", fbc_matting=False)
    assert torch.isfinite(out).all() and torch.equal(g.fg_frames, frames) and torch.equal(g.bg_frames, torch.flip(background, dims=[-1]))
    g2, out2, _, _, _ = _run(unet, vae, SimpleNamespace(estimate_alpha=no_alpha), bg_source="upload_flip", fbc_matting=False)
    assert torch.equal(out, out2)
    with pytest.raises(RuntimeError, match="fbc_matting"):              # matting on and no engine: an error, not a silent pass-through
        _run(unet, vae, None, bg_source="left")
    with pytest.raises(ValueError, match="bg_source upload"):           # upload without a background
        from tc_light_amd.generate import Generator
        gg = Generator(unet, vae, dict(iclight_model="fbc", fbc_matting=False, n_timesteps=1, apply_opt=False))
        gg.prepare_data(frames, None)


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_fbc(L, tmp_path):
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(__file__))
    import synth
    import run
    d = synth.video_clip(3, 64, 64, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    bgv = tmp_path / "bg.npy"
    np.save(bgv, (synth.video_clip(3, 64, 64, seed=4)["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{rgb_path: {vid}, height: 64, width: 64}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 1
  alpha_t: 0.01
  frame_range: [0, 3, 1]
  iclight_model: fbc
  bg_source: upload
  background_image_path: {bgv}
post_opt: {{apply_opt: false}}
models: {{allow_random: true}}
""")

    def run_once(*flags):
        cwd = os.getcwd()
        os.chdir(tmp_path)
        try:
            run.main(["--config", str(cfg), *flags])
        finally:
            os.chdir(cwd)
        outs = [os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "work") for f in fs if f == "output.npy"]
        assert len(outs) == 1
        out = np.load(outs[0])
        assert out.shape == (3, 64, 64, 3) and out.dtype == np.uint8
        return out, yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))["generation"]

    out, saved = run_once()                                            # a per-frame background: 3 frames for 3 frames
    assert (saved["iclight_model"], saved["bg_source"], saved["fbc_matting"]) == ("fbc", "upload", True)
