"""GPU: the light-direction / strength start (generation.init_latent, init_strength; IC-Light's "Lighting Preference", csrc/light.hip).
  * tcl_light_gradient_f32 and tcl_light_start_f16 against numpy, bit for bit (tests/light_refs.py);
  * the default (`init_latent: none`) draws and keeps what it did; an img2img start consumes the same draws;
  * the gradient through the real VAE engine against the f32 oracle (the encode tolerance of tests/test_gpu_vae.py: rel-L2 <= 1e-2;
    measured 1.3e-3 .. 1.8e-3 over the four sides);
  * the denoise loop entered mid-schedule against oracle/scheduler.py started at the same index (the bounds of tests/test_gpu_denoise_loop.py:
    fused prediction rel-L2 <= 1e-2, SDE update rel-L2 <= 2e-3; measured 3.3e-3 / 3.0e-3 / 3.1e-3 and 2.1e-4 / 2.1e-4 / 2.0e-4 over the three steps);
  * a two-rank split builds, block by block, the one-rank start; run.py end to end with --light / --strength.
Seeded random weights everywhere: parity and plumbing, not image quality."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import light_refs as R

pytestmark = pytest.mark.gpu
VAE_TOL = 1e-2                 # tests/test_gpu_vae.py, encode
EPS_TOL, STEP_TOL = 1e-2, 2e-3      # tests/test_gpu_denoise_loop.py


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


@pytest.fixture(scope="module")
def vae(L):
    from tc_light_amd import sd15
    from tc_light_amd.vae import VAEEngine
    sd = sd15.random_state_dict(sd15.vae_param_shapes(), seed=2)
    return sd, VAEEngine(sd, "cuda")


def st():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _stub_unet():
    """What Generator's constructor touches of a UNet engine; prepare_data / build_start never run it."""
    return SimpleNamespace(dev=torch.device("cuda"), tome=SimpleNamespace(args={}))


def _coefficients(n, s):
    from tc_light_amd import hostlogic as HL
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    sch = DPMSolverSDEScheduler()
    n_sched, begin, _ = HL.img2img_schedule(n, s)
    sch.set_timesteps(n_sched, begin)
    return tuple(float(np.float32(v)) for v in sch.add_noise_coefficients())


# ---------------------------------------------------------------------------------------------------------------- kernels, bit for bit
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (8, 9), (9, 8), (64, 255), (255, 256), (257, 64), (720, 1280)])
def test_gradient_bits(L, H, W):
    for k, side in enumerate(R.SIDES):
        out = torch.full((3 * H * W + 8,), -7.0, device="cuda")         # 8 guard floats behind the image
        L.tcl_light_gradient_f32(out, H, W, k, st())
        got = out.cpu().numpy()
        assert np.array_equal(got[:3 * H * W].reshape(3, H, W).view(np.uint32), R.gradient_image(side, H, W).view(np.uint32)), side
        assert (got[3 * H * W:] == -7.0).all(), side


def test_gradient_refuses_bad_arguments(L):
    out = torch.empty(3 * 4 * 4, device="cuda")
    for args in ((0, 4, 0), (4, 0, 0), (4, 4, 4), (4, 4, -1)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_light_gradient_f32(out, *args, st())


@pytest.mark.parametrize("N,h,w", [(1, 1, 1), (3, 5, 7), (2, 8, 8), (5, 90, 160)])
@pytest.mark.parametrize("ns", [(25, 0.9), (3, 0.6)])
def test_start_bits(L, N, h, w, ns):
    alpha, sigma_t = _coefficients(*ns)
    chw = 4 * h * w
    g = np.random.default_rng(N * 1000 + h)
    x0 = (g.standard_normal((N, chw)) * 0.8).astype(np.float16)
    z = g.standard_normal((N, chw)).astype(np.float32)
    x0[N // 2] = 0                                              # a frame of zeros: out = f16(sigma_t * z)
    x0[0, ::3] = 0
    z[0, :2], z[-1, -2:] = (4.0, -4.0), (-4.0, 4.0)
    xd, zd = torch.from_numpy(x0).cuda(), torch.from_numpy(z).cuda()
    for xs in (0, chw):
        for zs in (0, chw):
            out = torch.full((N * chw + 16,), 9.0, dtype=torch.float16, device="cuda")      # 16 guard halves behind the latents
            L.tcl_light_start_f16(out, xd, xs, zd, zs, N, chw, alpha, sigma_t, st())
            got = out.cpu().numpy()
            want = R.start(x0 if xs else x0[:1], z if zs else z[:1], alpha, sigma_t)
            want = np.broadcast_to(want, (N, chw))
            assert np.array_equal(got[:N * chw].reshape(N, chw).view(np.uint16), np.ascontiguousarray(want).view(np.uint16)), (xs, zs)
            assert (got[N * chw:] == 9.0).all(), (xs, zs)


def test_start_unaligned_pointers_and_bad_arguments(L):
    """A z block that starts 4 B off a 16 B boundary (a view into a larger tensor) takes the element-wise kernel: same bits."""
    alpha, sigma_t = _coefficients(25, 0.9)
    N, chw = 2, 256
    g = np.random.default_rng(5)
    x0, z = g.standard_normal((N, chw)).astype(np.float16), g.standard_normal(N * chw + 1).astype(np.float32)
    out = torch.empty(N, chw, dtype=torch.float16, device="cuda")
    zd = torch.from_numpy(z).cuda()
    L.tcl_light_start_f16(out, torch.from_numpy(x0).cuda(), chw, zd[1:], chw, N, chw, alpha, sigma_t, st())
    assert np.array_equal(out.cpu().numpy().view(np.uint16), R.start(x0, z[1:].reshape(N, chw), alpha, sigma_t).view(np.uint16))
    for xs, zs, n, c in ((8, chw, N, chw), (chw, -chw, N, chw), (chw, chw, 0, chw), (chw, chw, N, 0)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_light_start_f16(out, out, xs, zd, zs, n, c, alpha, sigma_t, st())


# ---------------------------------------------------------------------------------------------------------------- RNG: default unchanged, same draws
@pytest.mark.parametrize("mode", ["same", "vanilla"])
def test_default_start_and_rng_unchanged(L, mode):
    from tc_light_amd.generate import Generator
    n, hh, ww, seed = 3, 8, 8, 4321
    frames = torch.zeros(n, 3, 8 * hh, 8 * ww, device="cuda")
    base = dict(seed=seed, noise_mode=mode, max_tokens_per_pass=1 << 20)
    ga, gb = Generator(_stub_unet(), None, base), Generator(_stub_unet(), None, dict(base, init_latent="none", init_strength=0.5))
    ga.prepare_data(frames); gb.prepare_data(frames)
    assert ga.init_noise.dtype == torch.float16 and torch.equal(ga.init_noise, gb.init_noise)
    # what the parent commit drew, restated: one randn of [1 | n_total, 4, h, w] f32 on the device generator, times init_noise_sigma = 1, to f16
    rng = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(1 if mode == "same" else n, 4, hh, ww, generator=rng, device="cuda", dtype=torch.float32)
    assert torch.equal(ga.init_noise, z.to(torch.float16).expand(n, 4, hh, ww))
    nxt = [torch.randn(n, 4, hh, ww, generator=r, device="cuda") for r in (ga.rng_dev, gb.rng_dev, rng)]
    assert torch.equal(nxt[0], nxt[1]) and torch.equal(nxt[0], nxt[2])
    assert ga.schedule == (25, 0, 25) and gb.schedule == (25, 0, 25) and not gb.img2img


@pytest.mark.parametrize("mode", ["same", "vanilla"])
def test_light_start_consumes_the_default_draws(L, vae, mode):
    """Two generators, one seed: the `left` start is alpha*x0 + sigma_t*z with the z the default path drew, and both leave the RNG in one state.
    The default path keeps z as f16 (|z - z16| <= 2^-11 |z|) and the start is rounded to f16 once (<= 2^-11 |start|), so
    |start - (alpha*x0 + sigma_t*z16)| <= 2^-11 (sigma_t |z16| + |start|), with 1 % on top for the f32 arithmetic of both sides."""
    from tc_light_amd.generate import Generator
    n, hh, ww, seed = 3, 8, 8, 99
    frames = torch.zeros(n, 3, 8 * hh, 8 * ww, device="cuda")
    base = dict(seed=seed, noise_mode=mode, max_tokens_per_pass=1 << 20, n_timesteps=25)
    gd, gl = Generator(_stub_unet(), vae[1], base), Generator(_stub_unet(), vae[1], dict(base, init_latent="left", init_strength=0.9))
    gd.prepare_data(frames); gl.prepare_data(frames)
    assert gl.start_noise.dtype == torch.float32                # z stays f32 until the kernel
    start = gl.build_start(None).float()
    assert gl.schedule == (28, 3, 25) and gd.scheduler.init_noise_sigma == 1.0 and start.shape == (n, 4, hh, ww)
    alpha, sigma_t = _coefficients(25, 0.9)
    x0 = vae[1].encode(gl.light_gradient("left", 8 * hh, 8 * ww)).float()
    z16 = gd.init_noise.float()
    ref = alpha * x0 + sigma_t * z16
    bound = 2.0 ** -11 * (sigma_t * z16.abs() + ref.abs()) * 1.01 + 1e-7
    err = (start - ref).abs()
    print(f"[light start vs default draws, {mode}] max |start - ref| = {err.max().item():.3e}, max bound = {bound.max().item():.3e}")
    assert bool((err <= bound).all())
    # exactly: the same f32 z, redrawn from a generator of the same seed, through the numpy arithmetic
    rng = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(1 if mode == "same" else n, 4, hh, ww, generator=rng, device="cuda", dtype=torch.float32)
    want = R.start(x0.half().cpu().numpy(), z.cpu().numpy(), alpha, sigma_t)
    assert np.array_equal(gl.init_noise.cpu().numpy().view(np.uint16), np.ascontiguousarray(np.broadcast_to(want, (n, 4, hh, ww))).view(np.uint16))
    nxt = [torch.randn(n, 4, hh, ww, generator=r, device="cuda") for r in (gd.rng_dev, gl.rng_dev, rng)]
    assert torch.equal(nxt[0], nxt[1]) and torch.equal(nxt[0], nxt[2])


def test_latents_path_is_not_consulted(L, vae, tmp_path, capsys):
    from tc_light_amd.generate import Generator
    frames = torch.zeros(2, 3, 64, 64, device="cuda")
    cfg = dict(seed=1, init_latent="top", init_strength=0.5, n_timesteps=2, latents_path=str(tmp_path / "nowhere"), model_key="iclight",
               max_tokens_per_pass=1 << 20)
    g = Generator(_stub_unet(), vae[1], cfg)
    g.prepare_data(frames)
    out = capsys.readouterr().out
    assert out.count("[INFO]") == 1 and "latents_path is not consulted" in out and "latent path" not in out
    assert g.build_start(None).shape == (2, 4, 8, 8) and g.schedule == (4, 2, 2)
    for bad in (dict(init_latent="diagonal"), dict(init_strength=0.0), dict(init_strength=1.5), dict(init_strength=0.3, n_timesteps=1)):
        with pytest.raises(ValueError):
            Generator(_stub_unet(), vae[1], dict(cfg, **bad))


# ---------------------------------------------------------------------------------------------------------------- gradient through the VAE
@pytest.mark.parametrize("side", R.SIDES)
def test_gradient_latent_vs_oracle(L, vae, side):
    from oracle import sd15 as OS
    from tc_light_amd.generate import Generator
    sd, eng = vae
    g = Generator(_stub_unet(), eng, dict(max_tokens_per_pass=1 << 20))
    img = g.light_gradient(side, 64, 64)
    u = R.gradient_u8(side, 64, 64)
    assert np.array_equal(img.cpu().numpy()[0], R.gradient_image(side, 64, 64))
    got = eng.encode(img)
    # the oracle computes 2x - 1 itself: x = u/254 hands it the u/127 - 1 of the recipe (to an f32 ulp)
    x = torch.from_numpy(np.broadcast_to((u.astype(np.float64) / 254).astype(np.float32), (1, 3, 64, 64)).copy())
    assert float((2 * x.double() - 1 - torch.from_numpy(u / 127.0 - 1.0)).abs().max()) < 2e-7
    with torch.no_grad():
        want = OS.vae_encode(sd, x)
    r = rel(got.cpu(), want)
    print(f"[light gradient latent, {side}] rel-L2 vs the f32 oracle = {r:.3e}")
    assert got.shape == (1, 4, 8, 8) and got.dtype == torch.float16 and r < VAE_TOL, r


# ---------------------------------------------------------------------------------------------------------------- sharding
@pytest.mark.parametrize("init,mode", [("left", "vanilla"), ("source", "same")])
def test_two_rank_split_builds_the_one_rank_start(L, vae, init, mode):
    from tc_light_amd.generate import Generator
    from tc_light_amd.parallel import Dist
    n, hh, ww = 5, 8, 8                                         # blocks of 3 and 2 frames
    frames = torch.zeros(n, 3, 8 * hh, 8 * ww, device="cuda")
    cc = torch.randn(n, 4, hh, ww, generator=torch.Generator().manual_seed(8)).half().cuda()
    cfg = dict(seed=31, noise_mode=mode, init_latent=init, init_strength=0.6, n_timesteps=3, max_tokens_per_pass=1 << 20)
    one = Generator(_stub_unet(), vae[1], cfg)
    one.prepare_data(frames)
    whole = one.build_start(cc).clone()
    assert torch.isfinite(whole.float()).all() and float(whole.float().std()) > 0.1
    parts = []
    for rank in range(2):
        d = Dist(rank, 2)
        lo, hi = d.range(n)
        g = Generator(_stub_unet(), vae[1], cfg, dist=d)
        g.n_total = n
        g.prepare_data(frames[lo:hi])
        parts.append(g.build_start(cc[lo:hi]).clone())
    assert [p.shape[0] for p in parts] == [3, 2] and torch.equal(torch.cat(parts), whole)
    if mode == "vanilla":
        assert not torch.equal(whole[0], whole[1])
    if init == "source":                                        # the clean latents are really in it
        other = Generator(_stub_unet(), vae[1], cfg)
        other.prepare_data(frames)
        assert not torch.equal(other.build_start(cc.flip(0)), whole)


# ---------------------------------------------------------------------------------------------------------------- the loop, entered mid-schedule
def test_truncated_loop_vs_oracle(L, monkeypatch):
    """n_timesteps 3 at strength 0.6: 5 scheduler steps entered at index 2 -- a first-order step on an empty history, a second-order step whose
    history starts at index 2, the last step without noise.  Per step the oracle is fed what the engine had (as tests/test_gpu_denoise_loop.py)."""
    from oracle import pipeline as OP
    from oracle import sd15 as OS
    from oracle.scheduler import Scheduler as OSch
    from tc_light_amd import hostlogic as HL
    from tc_light_amd import sd15
    from tc_light_amd.generate import Generator
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe

    sd = sd15.random_state_dict(sd15.unet_param_shapes(), seed=1)
    eng = UNetEngine(sd, "cuda", VidToMe("cuda", seed=5, enabled=False))
    n, hh, ww = 6, 8, 8
    cfg = dict(n_timesteps=3, init_strength=0.6, init_latent="source", alpha_t=0.3, final_factor_t=0.5, win_size_t=4, chunk_size=4,
               guidance_scale=2.0, seed=77, noise_mode="vanilla")
    g = Generator(eng, None, cfg)
    assert g.schedule == (5, 2, 3)
    g.prepare_data(torch.zeros(n, 3, 8 * hh, 8 * ww, device="cuda"))
    gen = torch.Generator().manual_seed(3)
    conds = torch.randn(2, 154, 768, generator=gen).half()
    conds_t = torch.randn(2, 77, 768, generator=gen).half()
    cc = torch.randn(n, 4, hh, ww, generator=gen).half()
    x0 = g.build_start(cc.cuda()).clone()
    # the start is the add_noise of the first executed sigma, on the oracle's table
    osch = OSch(5)
    osch.i = 2
    s2 = float(osch.sigmas[2])
    a2 = 1.0 / (s2 * s2 + 1.0) ** 0.5
    z0 = torch.randn(n, 4, hh, ww, generator=torch.Generator(device="cuda").manual_seed(77), device="cuda").cpu()
    assert rel(x0.cpu(), a2 * cc.float() + s2 * a2 * z0) < 2e-3          # f16 storage

    zs, seen, alphas_used = [], [], []
    step = g.scheduler.step

    def recording_step(eps, t, x, noise=None, **kw):
        zs.append(None if noise is None else noise.float().cpu())
        seen.append((x.float().cpu(), eps.float().cpu()))          # latents entering the step, fused noise prediction
        return step(eps, t, x, noise=noise, **kw)
    g.scheduler.step = recording_step
    fuse = g.L.tcl_adain_fuse_f16

    def recording_fuse(*a):
        alphas_used.append(a[4])
        return fuse(*a)
    monkeypatch.setattr(g.L, "tcl_adain_fuse_f16", recording_fuse)
    x_hip = g.ddim_sample(x0.clone(), conds.cuda(), conds_t.cuda(), cc.cuda()).float().cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(x_hip).all() and len(zs) == 3 and zs[-1] is None and all(z is not None for z in zs[:2])
    assert alphas_used == HL.alpha_schedule(0.3, 0.5, 3)           # the decay over the EXECUTED steps, counted from 0
    assert g.scheduler.timesteps.tolist() == osch.timesteps[2:].tolist() and len(g.scheduler.timesteps) == 3

    c = g.cfg
    alphas = OP.alpha_schedule(c.alpha_t, c.final_factor_t, 3)
    assert list(alphas) == alphas_used
    xy_s = HL.ChunkSampler(c.seed, c.chunk_size, c.merge_global, c.chunk_ord)          # rank 0: seed + 7919 * 0
    yt_s = HL.ChunkSampler(c.seed + 1, c.chunk_size, c.merge_global, c.chunk_ord)
    ccf, text, text_t = cc.float(), conds.float(), conds_t.float()

    def pred(xin, txt, t):
        return OP.cfg(OS.unet_forward(sd, torch.cat([xin, xin]), t, txt), c.guidance_scale)

    def fused_eps(xc, xy_chunks, yt_chunks, i, t):
        noises = torch.zeros_like(xc)
        for ch in xy_chunks:
            noises[ch] = pred(torch.cat([xc[ch], ccf[ch]], 1), text, float(t))
        return OP.temporal_denoise(xc, ccf, alphas[i], noises, c.win_size_t, [torch.as_tensor(ch) for ch in yt_chunks],
                                   lambda xt, ct, ch, sl: pred(torch.cat([xt, ct], 1), text_t, float(t)))[1]

    nxt = [seen[1][0], seen[2][0], x_hip]                      # latents the engine had after each step
    with torch.no_grad():
        for i, t in enumerate(osch.timesteps[2:].tolist()):
            xy_chunks, yt_chunks = xy_s.get_chunks(n), yt_s.get_chunks(ww)
            r = rel(seen[i][1], fused_eps(seen[i][0], xy_chunks, yt_chunks, i, t))
            print(f"[truncated loop parity] step {i} (sigma index {2 + i}): fused eps rel-L2 = {r:.3e}")
            assert r < EPS_TOL, (i, r)
            z = zs[i] if zs[i] is not None else torch.zeros_like(seen[i][0])
            assert osch.i == 2 + i
            r = rel(nxt[i], osch.step(seen[i][1], seen[i][0], z))
            print(f"[truncated loop parity] step {i} (sigma index {2 + i}): latents after the SDE step rel-L2 = {r:.3e}")
            assert r < STEP_TOL, (i, r)


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_with_light_and_strength(L, tmp_path):
    """run.py on the clip and stand-in weights of tests/test_gpu_run.py (4 frames of 192x256), 2 steps, with and without --light left --strength 0.5."""
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    import synth
    import run
    d = synth.video_clip(4, 192, 256, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
data: {{rgb_path: {vid}, height: 192, width: 256}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 2
  alpha_t: 0.01
  frame_range: [0, 4, 1]
post_opt: {{apply_opt: false}}
models: {{allow_random: true}}
""")                                                            # stage 1 / 2 off: the start and the loop are what this run is about
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        res = {}
        for name, extra in (("light", ["--light", "left", "--strength", "0.5"]), ("plain", [])):
            work = tmp_path / f"work_{name}"
            one = tmp_path / f"{name}.yaml"
            one.write_text(cfg.read_text() + f"work_dir: {work}\n")
            run.main(["--config", str(one)] + extra)
            outs = [os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs if f == "output.npy"]
            assert len(outs) == 1
            out = np.load(outs[0])
            assert out.shape == (4, 192, 256, 3) and out.dtype == np.uint8
            res[name] = (out, yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))["generation"])
    finally:
        os.chdir(cwd)
    gl, gp = res["light"][1], res["plain"][1]
    assert (gl["init_latent"], gl["init_strength"], gl["scheduler_steps"], gl["steps_executed"]) == ("left", 0.5, 4, 2)
    assert (gl["scheduler_steps"], 4 - gl["steps_executed"], gl["steps_executed"]) == R.schedule(2, 0.5)
    assert (gp["init_latent"], gp["init_strength"], gp["scheduler_steps"], gp["steps_executed"]) == ("none", 0.9, 2, 2)
    diff = np.abs(res["light"][0].astype(np.int32) - res["plain"][0].astype(np.int32))
    print(f"[run.py --light left --strength 0.5] mean |difference to the plain run| = {diff.mean():.3f} of 255")
    assert diff.max() > 0
