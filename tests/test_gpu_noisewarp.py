"""generation.noise_mode warp on the GPU: tcl_noise_warp_count and tcl_noise_warp_apply_f32 against the numpy reference (tests/noisewarp_refs.py) bit for
bit -- k, the fixed-point sums, the field F_t and the latent noise z_t of every frame, on every flow case of the reference's table at 64x64 and 72x136
(non-square, 9 latent rows, a partial tile) -- two runs of one chain against each other, the statistics at 256x256, the wrapper and the refusals, then
the Generator with stub engines (start noise, img2img start, two-rank split, per-step noise, same / vanilla untouched) and run.py --noise_mode warp.
Outputs sit between sentinel guards."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import noisewarp_refs as R

pytestmark = pytest.mark.gpu

H16 = torch.float16
GUARD = 256
SENT = 0x7FC12345                                  # a NaN bit pattern no arithmetic here produces
SHAPES = [(64, 64), (72, 136)]
NAMES = ["zero", "integer", "half", "zoom_in", "zoom_out", "one_source", "nonfinite", "mask_edge"]
N = 4


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def guards_kept(buf, n):
    return bool((buf[:GUARD] == SENT).all() and (buf[GUARD + n:] == SENT).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def direct(L, G, flows, masks):
    """The two C entries frame by frame on host arrays -> (z [N,4,h,w], [F_t], [k_t], [S_t]) on the host, as noisewarp_refs.chain(detail=True)."""
    n, _, H, W = G.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (G, flows, masks)]
    ws_bytes = L.tcl_noise_warp_workspace_bytes(H, W)
    assert ws_bytes == 36 * H * W
    wbuf, ws = guarded((ws_bytes // 4,), torch.int32)
    fb = [guarded((4, H, W)) for _ in range(2)]
    zbuf, z = guarded((n, 4, H // 8, W // 8))
    Fs, ks, Ss = [], [], []
    for t in range(n):
        (pbuf, prev), (cbuf, cur) = fb[(t + 1) & 1], fb[t & 1]
        if t > 0:
            L.tcl_noise_warp_count(dev[1], dev[2], dev[0][t], t, n, H, W, ws, ws_bytes, st())
        L.tcl_noise_warp_apply_f32(dev[1], dev[2], dev[0][t], prev, cur, z, t, n, H, W, ws, ws_bytes, st())
        torch.cuda.synchronize()
        Fs.append(cur.cpu().numpy().copy())
        raw = ws.cpu().numpy()
        Ss.append(None if t == 0 else raw[:8 * H * W].view(np.int64).reshape(4, H, W).copy())
        ks.append(None if t == 0 else raw[8 * H * W:].reshape(H, W).copy())
        assert guards_kept(wbuf, ws.numel()) and guards_kept(pbuf, prev.numel()) and guards_kept(cbuf, cur.numel()) and guards_kept(zbuf, z.numel())
        if t == 0:
            assert bool((wbuf == SENT).all()), "frame 0 touched the workspace"
    for d, a in zip(dev, (G, flows, masks)):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), bits(a)), "an input was written"
    return z.cpu().numpy(), Fs, ks, Ss


_cache = {}


def reference(H, W, name):
    """The case and its reference, computed once and shared."""
    if (H, W) not in _cache:
        _cache[(H, W)] = (R.fields(N, H, W, seed=H + W), R.cases(N, H, W), {})
    G, cases, done = _cache[(H, W)]
    if name not in done:
        done[name] = R.chain(G, *cases[name], detail=True)
    return G, cases[name], done[name]


# ---------------------------------------------------------------------------------------------------------------- the kernels, bit for bit
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_chain_bits(L, H, W, name):
    G, (flows, masks), (z_ref, F_ref, k_ref, S_ref) = reference(H, W, name)
    z, Fs, ks, Ss = direct(L, G, flows, masks)
    for t in range(N):
        if t > 0:
            assert np.array_equal(ks[t], k_ref[t]), (name, t, "k")
            assert np.array_equal(Ss[t], S_ref[t]), (name, t, "sums")
        assert np.array_equal(bits(Fs[t]), bits(F_ref[t])), (name, t, "F")
        assert np.array_equal(bits(z[t]), bits(z_ref[t])), (name, t, "z")
    kmax = max(int(k.max()) for k in k_ref[1:])
    print(f"{name} {H}x{W}: k up to {kmax}, valid share {np.mean([k.sum() / (H * W) for k in k_ref[1:]]):.3f}")
    if name == "one_source":
        assert kmax == H * W
    if name == "zero":
        assert all(np.array_equal(bits(z[t]), bits(z[0])) for t in range(1, N))


@pytest.mark.parametrize("name", ["one_source", "zoom_in", "nonfinite"])
def test_two_runs_of_one_chain_are_the_same_bits(L, name):
    H, W = SHAPES[1]
    G, (flows, masks), _ = reference(H, W, name)
    a, b = direct(L, G, flows, masks), direct(L, G, flows, masks)
    assert np.array_equal(bits(a[0]), bits(b[0]))
    for t in range(1, N):
        assert np.array_equal(bits(a[1][t]), bits(b[1][t])) and np.array_equal(a[2][t], b[2][t]) and np.array_equal(a[3][t], b[3][t])


def _recording_draw(seed):
    from tc_light_amd.noisewarp import field_draw
    rng = torch.Generator(device="cuda").manual_seed(seed)
    draw, seen = field_draw(rng, torch.device("cuda")), []

    def rec(H, W):
        seen.append(draw(H, W))
        return seen[-1]
    return rec, seen


def test_wrapper_and_statistics_at_256(L):
    """warp_chain on device draws under a 2x zoom, five frames: the reference's bits on the same draws, and white unit-variance latent noise in
    every frame (the bounds of tests/test_noisewarp_refs_cpu.py, n = 4096)."""
    from tc_light_amd.noisewarp import warp_chain
    n, H, W = 5, 256, 256
    flows, masks = R.zoom(n, H, W, 2.0), R.ones(n, H, W)
    rec, seen = _recording_draw(3)
    z = warp_chain(rec, torch.from_numpy(flows).cuda(), torch.from_numpy(masks).cuda(), n, H, W)
    torch.cuda.synchronize()
    assert len(seen) == n and tuple(z.shape) == (n, 4, 32, 32) and z.dtype == torch.float32
    z = z.cpu().numpy()
    want = R.chain(np.stack([g.cpu().numpy() for g in seen]), flows, masks)
    assert np.array_equal(bits(z), bits(want))
    bm, bv = R.bounds(z[0].size)
    for t in range(n):
        m, v, ch, cv = R.stats(z[t])
        print(f"frame {t}: mean {m:+.4f} var {v:.4f} cov h {ch:+.4f} v {cv:+.4f}  (bounds {bm:.4f} / {bv:.4f})")
        assert abs(m) <= bm and abs(v - 1.0) <= bv and abs(ch) <= bm and abs(cv) <= bm


def test_refusals(L):
    from tc_light_amd.noisewarp import warp_chain
    H, W, n = 16, 24, 2
    f, m = torch.zeros(n, 2, H, W, device="cuda"), torch.ones(n, 1, H, W, device="cuda")
    G = torch.zeros(4, H, W, device="cuda")
    fbuf, F = guarded((4, H, W))
    pbuf, P = guarded((4, H, W))
    zbuf, z = guarded((n, 4, H // 8, W // 8))
    nb = L.tcl_noise_warp_workspace_bytes(H, W)
    wbuf, ws = guarded((nb // 4,), torch.int32)
    assert nb == 36 * H * W and L.tcl_noise_warp_workspace_bytes(12, 24) == 0 and L.tcl_noise_warp_workspace_bytes(16, 0) == 0
    ok_c = dict(f=f, m=m, G=G, t=1, N=n, H=H, W=W, ws=ws, nb=nb)
    ok_a = dict(ok_c, P=P, F=F, z=z)
    for change in (dict(t=0), dict(t=n), dict(H=12), dict(W=20), dict(nb=nb - 1), dict(ws=ws[1:]), dict(f=0), dict(m=0), dict(G=0), dict(ws=0), dict(N=0)):
        a = dict(ok_c, **change)
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_noise_warp_count(a["f"], a["m"], a["G"], a["t"], a["N"], a["H"], a["W"], a["ws"], a["nb"], st())
    for change in (dict(t=-1), dict(t=n), dict(H=12), dict(W=20), dict(nb=nb - 1), dict(ws=ws[1:]), dict(f=0), dict(m=0), dict(G=0), dict(P=0), dict(F=0),
                   dict(z=0), dict(ws=0), dict(P=F), dict(P=G), dict(F=G)):
        a = dict(ok_a, **change)
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_noise_warp_apply_f32(a["f"], a["m"], a["G"], a["P"], a["F"], a["z"], a["t"], a["N"], a["H"], a["W"], a["ws"], a["nb"], st())
    torch.cuda.synchronize()
    for buf in (fbuf, pbuf, zbuf, wbuf):
        assert bool((buf == SENT).all()), "a refused call wrote something"
    draw = lambda H, W: torch.zeros(4, H, W, device="cuda")
    for args in ((f[:, :1].contiguous(), m, n, H, W), (f, m[:1], n, H, W), (f.double(), m, n, H, W), (f.cpu(), m.cpu(), n, H, W), (f, m, n, 12, 24)):
        with pytest.raises(ValueError, match="noise_mode warp"):
            warp_chain(draw, *args)


# ---------------------------------------------------------------------------------------------------------------- the Generator
def _stub_unet():
    """What Generator's constructor and a ddim_sample without its UNet passes touch of a UNet engine."""
    return SimpleNamespace(dev=torch.device("cuda"), tome=SimpleNamespace(args={}, reset_global_tokens=lambda: None))


def _flows(n, H=64, W=64):
    f, m = R.cases(n, H, W)["zoom_in"]
    return torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda()


def _chain(seed, pf, mk, n, H=64, W=64, chains=1):
    """What a Generator seeded with `seed` must draw: `chains` chains, one after the other, from one device generator."""
    from tc_light_amd.noisewarp import field_draw, warp_chain
    rng = torch.Generator(device="cuda").manual_seed(seed)
    return [warp_chain(field_draw(rng, torch.device("cuda")), pf, mk, n, H, W) for _ in range(chains)]


@pytest.fixture(scope="module")
def vae(L):
    from tc_light_amd import sd15
    from tc_light_amd.vae import VAEEngine
    return VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")


def _gen(n, pf, mk, vae=None, dist=None, n_total=None, **over):
    from tc_light_amd.generate import Generator
    g = Generator(_stub_unet(), vae, dict(dict(seed=77, n_timesteps=3, noise_mode="warp", max_tokens_per_pass=1 << 20), **over), dist=dist)
    if n_total is not None:
        g.n_total = n_total
    g.prepare_data(torch.zeros(n, 3, 64, 64, device="cuda"), past_flows=pf, mask_bwds=mk)
    return g


def test_generator_start_is_the_chain(L):
    n = 4
    pf, mk = _flows(n)
    g = _gen(n, pf, mk)
    z, = _chain(77, pf, mk, n)
    assert g.init_noise.dtype == H16 and tuple(g.init_noise.shape) == (n, 4, 8, 8)
    assert torch.equal(g.init_noise, (z * g.scheduler.init_noise_sigma).to(H16))
    assert not torch.equal(g.init_noise[0], g.init_noise[1])
    from tc_light_amd.generate import Generator
    with pytest.raises(ValueError, match="generation.noise_mode warp"):
        Generator(_stub_unet(), None, dict(noise_mode="warp")).prepare_data(torch.zeros(n, 3, 64, 64, device="cuda"))
    with pytest.raises(ValueError, match="generation.noise_mode warp"):
        _gen(n, pf[:3], mk[:3])
    with pytest.raises(NotImplementedError):
        Generator(_stub_unet(), None, dict(noise_mode="mixed")).prepare_data(torch.zeros(n, 3, 64, 64, device="cuda"), past_flows=pf, mask_bwds=mk)


def test_generator_img2img_start_is_the_noised_chain(L, vae):
    n = 3
    pf, mk = _flows(n)
    g = _gen(n, pf, mk, vae=vae, init_latent="left", init_strength=0.5)
    got = g.build_start(None).clone()
    z, = _chain(77, pf, mk, n)
    assert torch.equal(g.start_noise, z)
    x0 = vae.encode(g.light_gradient("left", 64, 64)).contiguous()
    want = g._noised_start(n, x0, 0, z, g.schedule)
    assert got.dtype == H16 and tuple(got.shape) == (n, 4, 8, 8) and torch.equal(got, want)
    assert not torch.equal(got[0], got[1])


def test_two_rank_split_concatenates_to_the_one_rank_start(L):
    from tc_light_amd.parallel import Dist
    n = 5
    pf, mk = _flows(n)
    whole = _gen(n, pf, mk).init_noise
    parts = []
    for rank in range(2):
        d = Dist(rank, 2)
        lo, hi = d.range(n)
        parts.append(_gen(hi - lo, pf, mk, dist=d, n_total=n).init_noise)
    assert [p.shape[0] for p in parts] == [3, 2] and torch.equal(torch.cat(parts), whole)


def _step_noise(g, n):
    """ddim_sample without its UNet passes: what sch.step is handed as noise at every step."""
    seen = []
    step = g.scheduler.step
    g._unet_xy = lambda *a, **k: None
    g.scheduler.step = lambda eps, t, x, noise=None, **k: seen.append(None if noise is None else noise.clone()) or step(eps, t, x, noise=noise, **k)
    try:
        g.ddim_sample(g.init_noise.clone(), None, None, torch.zeros(n, 4, 8, 8, dtype=H16, device="cuda"))
    finally:
        g.scheduler.step = step
        del g._unet_xy
    torch.cuda.synchronize()
    return seen


def test_per_step_noise(L):
    n = 4
    pf, mk = _flows(n)
    chains = _chain(77, pf, mk, n, chains=3)                    # the start, then one chain per step that adds noise
    seen = _step_noise(_gen(n, pf, mk), n)
    assert len(seen) == 3 and seen[2] is None                   # the last SDE step adds none
    for i in range(2):
        assert seen[i].dtype == H16 and torch.equal(seen[i], chains[1 + i].to(H16))
    # steps false: today's draws behind the start's chain
    seen = _step_noise(_gen(n, pf, mk, noise_warp=dict(steps=False)), n)
    from tc_light_amd.noisewarp import field_draw, warp_chain
    rng = torch.Generator(device="cuda").manual_seed(77)
    warp_chain(field_draw(rng, torch.device("cuda")), pf, mk, n, 64, 64)
    for i in range(2):
        assert torch.equal(seen[i], torch.randn(n, 4, 8, 8, generator=rng, device="cuda", dtype=torch.float32).to(H16))
    assert seen[2] is None


@pytest.mark.parametrize("mode", ["same", "vanilla"])
def test_same_and_vanilla_draw_what_they_drew(L, mode):
    """The stream of rng_dev under the two existing modes, flows handed in or not: one start draw of the mode's shape, then one [n_total,4,h,w] draw
    per step, and nothing else."""
    from tc_light_amd.parallel import Dist
    n = 5
    pf, mk = _flows(n)
    for hand_in in (False, True):
        for rank, world in ((0, 1), (1, 2)):
            d = Dist(rank, world)
            lo, hi = d.range(n)
            g = _gen(hi - lo, pf if hand_in else None, mk if hand_in else None, dist=d, n_total=n, noise_mode=mode, noise_warp=dict(steps=True))
            rng = torch.Generator(device="cuda").manual_seed(77)
            if mode == "same":
                start = torch.randn(1, 4, 8, 8, generator=rng, device="cuda", dtype=torch.float32).to(H16).expand(hi - lo, -1, -1, -1)
            else:
                start = torch.randn(n, 4, 8, 8, generator=rng, device="cuda", dtype=torch.float32)[lo:hi].to(H16)
            assert g.cfg.noise_warp is None and g.warp_flows is None and torch.equal(g.init_noise, start)
            seen = _step_noise(g, hi - lo)
            for i in range(2):
                assert torch.equal(seen[i], torch.randn(n, 4, 8, 8, generator=rng, device="cuda", dtype=torch.float32)[lo:hi].to(H16))
            assert seen[2] is None
            assert torch.equal(torch.randn(4, generator=g.rng_dev, device="cuda"), torch.randn(4, generator=rng, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- run.py
def _run_config(tmp_path, root, vid, name):
    work = tmp_path / f"work_{name}"
    cfg = tmp_path / f"{name}.yaml"
    cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {work}
data: {{rgb_path: {vid}, height: 64, width: 64}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 2
  frame_range: [0, 4, 1]
post_opt: {{apply_opt: false}}
models: {{allow_random: true}}
""")
    return work, cfg


def test_run_py_with_noise_mode_warp(L, tmp_path):
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path.insert(0, root)
    import synth
    import run
    d = synth.video_clip(4, 64, 64, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    # the flows come from the on-disk cache (no estimator takes a 64x64 frame): the reference's layout, one [1,2,H,W] tensor per frame
    rng = torch.Generator().manual_seed(1)
    for kind in ("future", "past"):
        os.makedirs(tmp_path / f"clip_{kind}_flow_memflow")
        for i in range(4):
            torch.save(torch.randn(1, 2, 64, 64, generator=rng) * 2, tmp_path / f"clip_{kind}_flow_memflow" / f"{i:04d}.pt")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        seen = []
        from tc_light_amd import noisewarp
        real_chain = noisewarp.warp_chain
        noisewarp.warp_chain = lambda *a, **k: seen.append(1) or real_chain(*a, **k)
        try:
            work, cfg = _run_config(tmp_path, root, vid, "warp")
            run.main(["--config", str(cfg), "--noise_mode", "warp"])
        finally:
            noisewarp.warp_chain = real_chain
        assert len(seen) == 2                                   # the start and the one step that adds noise
        outs = [os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs if f == "output.npy"]
        assert len(outs) == 1
        out = np.load(outs[0])
        assert out.shape == (4, 64, 64, 3) and out.dtype == np.uint8
        rec = yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))
        assert rec["generation"]["noise_mode"] == "warp" and rec["generation"]["noise_warp"] == dict(steps=True)
        # out of scope beside the mode: refused before any model is loaded
        loaded = []
        real = run.init_iclight
        run.init_iclight = lambda *a, **k: loaded.append(1) or real(*a, **k)
        try:
            for name, lines, word in (("keys", ["--keyframes", "2"], "generation.keyframes"),
                                      ("highres", ["--highres_scale", "2"], "generation.highres_scale"),
                                      ("normal", ["--normal", "--iclight_model", "fbc"], "generation.normal")):
                work, cfg = _run_config(tmp_path, root, vid, name)
                with pytest.raises(ValueError) as e:
                    run.main(["--config", str(cfg), "--noise_mode", "warp"] + lines)
                assert "generation.noise_mode" in str(e.value) and word in str(e.value), str(e.value)
        finally:
            run.init_iclight = real
        assert loaded == []
    finally:
        os.chdir(cwd)
