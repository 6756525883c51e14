"""GPU: the animated light (generation.light_path; tcl_light_ramp_angle_f32 in csrc/light.hip, Generator.light_ramps).
  * the kernel against the numpy f64 restatement (tests/sweep_refs.py), bit for bit: scalar and 16 B path, four frames per launch, both level pairs,
    the three planes, sentinel floats behind the image;
  * the kernel at 0 / 90 / 180 / 270 against tcl_light_gradient_f32 / tcl_bg_ramp_f32: at most one level, sizes with a single sample along the
    ramp's axis (R == 0) included; the count of differing pixels is printed;
  * the refusals; light_ramps renders every distinct angle once;
  * fc: a constant path at 0 is the `init_latent: left` run bit for bit (start latents and relit frames); a sweep gives every frame the start of its
    own angle; a two-rank split builds the one-rank start;
  * fbc: a constant path at 180 is the `bg_source: right` run bit for bit; a sweep hands the loop one background latent per frame, each the encode
    of its ramp alone;
  * run.py --light_sweep end to end, and what config.yaml records.
Seeded random weights everywhere: parity and plumbing, not image quality."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import sweep_refs as R

pytestmark = pytest.mark.gpu
H16 = torch.float16
EINVAL = "TCL_EINVAL"


@pytest.fixture(scope="module", autouse=True)
def _leave_no_garbage():
    """Set up first, so torn down after the engines of this module are released: what they held goes back now, not in the middle of a later test
    that watches torch.cuda.memory_allocated()."""
    yield
    import gc
    gc.collect()


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
    return VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")


def _unet(in_channels):
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    shapes = sd15.unet_param_shapes() if in_channels == 8 else sd15.unet_param_shapes(in_channels=in_channels)
    return UNetEngine(sd15.random_state_dict(shapes, seed=1), "cuda", VidToMe("cuda", seed=5))


@pytest.fixture(scope="module")
def unet8(L):
    return _unet(8)


@pytest.fixture(scope="module")
def unet12(L):
    return _unet(12)


def st():
    return torch.cuda.current_stream().cuda_stream


def _stub_unet():
    """What Generator's constructor touches of a UNet engine; prepare_data / build_start never run it."""
    return SimpleNamespace(dev=torch.device("cuda"), tome=SimpleNamespace(args={}))


def _ramps(L, dirs, H, W, hi, lo, guard=8):
    """One launch over len(dirs) frames -> ([N,3,H,W] f32 numpy, the guard floats behind it)."""
    N = len(dirs)
    out = torch.full((N * 3 * H * W + guard,), -7.0, device="cuda")
    d = torch.tensor(dirs, dtype=torch.float64).cuda()
    L.tcl_light_ramp_angle_f32(out, d, N, H, W, hi, lo, st())
    got = out.cpu().numpy()
    return got[:N * 3 * H * W].reshape(N, 3, H, W), got[N * 3 * H * W:]


# ---------------------------------------------------------------------------------------------------------------- the kernel, bit for bit
@pytest.mark.parametrize("hi,lo", R.LEVELS)
@pytest.mark.parametrize("H,W", R.SIZES)
def test_ramp_angle_bits(L, H, W, hi, lo):
    from tc_light_amd import hostlogic as HL
    assert HL.light_dirs(list(R.ANGLES)) == R.dirs(list(R.ANGLES))
    for angles in (R.ANGLES[:4], R.ANGLES[2:]):                 # four frames per launch, every angle of the list in one of the two
        dirs = R.dirs(list(angles))
        got, guard = _ramps(L, dirs, H, W, hi, lo)
        for k, (c, s) in enumerate(dirs):
            want = R.ramp_image(c, s, H, W, hi, lo)
            assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), (angles[k], H, W)
            assert np.array_equal(got[k, 0], got[k, 1]) and np.array_equal(got[k, 0], got[k, 2])
        assert (guard == -7.0).all()


def test_ramp_angle_more_than_one_block_and_a_misaligned_output(L):
    """65 x 96 = 6240 pixels, three frames: 19 blocks of the 16 B path; the same call into a buffer 4 B off a 16 B boundary takes the scalar path: same bits."""
    H, W, hi, lo = 65, 96, 255, 0
    dirs = R.dirs([200.25, 37.5, 359.999])
    want = np.stack([R.ramp_image(c, s, H, W, hi, lo) for c, s in dirs])
    got, guard = _ramps(L, dirs, H, W, hi, lo)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (guard == -7.0).all()
    buf = torch.full((3 * 3 * H * W + 9,), -7.0, device="cuda")
    L.tcl_light_ramp_angle_f32(buf[1:], torch.tensor(dirs, dtype=torch.float64).cuda(), 3, H, W, hi, lo, st())
    off = buf.cpu().numpy()
    assert off[0] == -7.0 and (off[1 + 9 * H * W:] == -7.0).all()
    assert np.array_equal(off[1:1 + 9 * H * W].reshape(3, 3, H, W).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("H,W", R.SIZES)
def test_axis_angles_against_the_existing_ramp_kernels(L, H, W):
    axis = (0.0, 90.0, 180.0, 270.0)
    sides = {0.0: 0, 90.0: 2, 180.0: 1, 270.0: 3}               # TCL_LIGHT_LEFT, TOP, RIGHT, BOTTOM
    worst = 0
    for hi, lo in R.LEVELS:
        got, _ = _ramps(L, R.dirs(list(axis)), H, W, hi, lo)
        for k, a in enumerate(axis):
            old = torch.empty(3 * H * W, device="cuda")
            if (hi, lo) == (255, 0):
                L.tcl_light_gradient_f32(old, H, W, sides[a], st())
            else:
                start, stop = (hi, lo) if a in (0.0, 90.0) else (lo, hi)
                L.tcl_bg_ramp_f32(old, H, W, sides[a], start, stop, st())
            u_old = np.rint(254 * old.cpu().numpy().astype(np.float64)).astype(np.int64).reshape(3, H, W)
            u_new = np.rint(254 * got[k].astype(np.float64)).astype(np.int64)
            assert np.array_equal(u_old[0], R.linspace_u8(a, H, W, hi, lo))
            diff = np.abs(u_new - u_old)
            print(f"[angle kernel vs the existing ramps] {H}x{W} levels ({hi}, {lo}) angle {a:g}: max |difference| = {diff.max()} levels, "
                  f"{int((diff[0] > 0).sum())} of {H * W} pixels differ")
            worst = max(worst, int(diff.max()))
    assert worst <= 1, worst


def test_ramp_angle_refusals(L):
    H, W = 4, 4
    out = torch.full((2 * 3 * H * W,), -7.0, device="cuda")
    d = torch.tensor([(1.0, 0.0), (0.0, 1.0)], dtype=torch.float64).cuda()
    for args in ((0, d, 2, H, W, 255, 0), (out, 0, 2, H, W, 255, 0), (out, d, 0, H, W, 255, 0), (out, d, -1, H, W, 255, 0),
                 (out, d, 2, 0, W, 255, 0), (out, d, 2, H, 0, 255, 0), (out, d, 2, H, -3, 255, 0),
                 (out, d, 2, 1 << 14, 1 << 15, 255, 0),           # 3 * 2 * 2^29 >= 2^31
                 (out, d, 1, 1 << 15, (1 << 16) // 3 + 1, 255, 0),      # 3 * 1 * H * W just past 2^31
                 (out, d, 2, H, W, 256, 0), (out, d, 2, H, W, 255, -1), (out, d, 2, H, W, 300, 280), (out, d, 2, H, W, -2, -5),
                 (out, d, 2, H, W, 32, 224)):                      # hi < lo
        with pytest.raises(RuntimeError, match=EINVAL):
            L.tcl_light_ramp_angle_f32(*args, st())
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                   # a refusal writes nothing
    L.tcl_light_ramp_angle_f32(out, d, 2, H, W, 64, 64, st())       # hi == lo: a flat image
    assert np.array_equal(out.cpu().numpy(), np.full(2 * 3 * H * W, np.float32(64) / np.float32(254), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- light_ramps
def test_light_ramps_renders_every_distinct_angle_once(L, monkeypatch):
    from tc_light_amd.generate import Generator
    g = Generator(_stub_unet(), None, dict(max_tokens_per_pass=1 << 20))
    calls = []
    real = g.L.tcl_light_ramp_angle_f32

    def counting(*a):
        calls.append(a[2])
        return real(*a)
    monkeypatch.setattr(g.L, "tcl_light_ramp_angle_f32", counting)
    H, W = 17, 33
    for hi, lo in R.LEVELS:
        del calls[:]
        imgs, index = g.light_ramps([30.0, 30.0, 90.0, 30.0, 90.0], H, W, hi, lo)
        assert tuple(imgs.shape) == (2, 3, H, W) and imgs.dtype == torch.float32 and index == [0, 0, 1, 0, 1] and calls == [1]
        (c, s), = R.dirs([30.0])
        assert np.array_equal(imgs[0].cpu().numpy().view(np.uint32), R.ramp_image(c, s, H, W, hi, lo).view(np.uint32))
        top = R.linspace_u8(90.0, H, W, hi, lo).astype(np.float32) / np.float32(254)      # the existing kernel's image, not the formula's
        assert np.array_equal(imgs[1].cpu().numpy(), np.broadcast_to(top, (3, H, W)))
    del calls[:]
    imgs, index = g.light_ramps([390.0, 30.0, -330.0, 45.0, 0.0, 360.0, 200.25, 45.0], H, W, 255, 0)      # equal after the reduction: one image
    assert tuple(imgs.shape) == (4, 3, H, W) and index == [0, 0, 0, 1, 2, 2, 3, 1] and calls == [3]      # 30, 45, 200.25 in ONE launch; 0 is `left`
    assert torch.equal(imgs[2:3], g.light_gradient("left", H, W))
    del calls[:]
    imgs, index = g.light_ramps([180.0, 180.0], H, W, 224, 32)      # axis-aligned only: no launch of the new kernel at all
    assert calls == [] and index == [0, 0] and torch.equal(imgs, g.bg_ramp("right", H, W))
    imgs, index = g.light_ramps([10.0, 20.0, 30.0], 24, 40, 255, 0)      # nothing axis-aligned: the launch's own buffer
    assert tuple(imgs.shape) == (3, 3, 24, 40) and index == [0, 1, 2]


# ---------------------------------------------------------------------------------------------------------------- fc: the start latents
FC = dict(seed=99, n_timesteps=2, init_strength=0.5, max_tokens_per_pass=1 << 20)


def _start(vae, n, dist=None, n_total=None, frames=None, **over):
    from tc_light_amd.generate import Generator
    g = Generator(_stub_unet(), vae, dict(FC, **over), dist=dist)
    if n_total is not None:
        g.n_total = n_total
    g.prepare_data(torch.zeros(n, 3, 64, 64, device="cuda") if frames is None else frames)
    return g, g.build_start(None).clone()


@pytest.mark.parametrize("mode", ["same", "vanilla"])
def test_constant_path_is_the_init_latent_start(L, vae, mode):
    for angle, side in ((0, "left"), (90, "top"), (180.0, "right"), (-90, "bottom"), (720, "left")):
        gp, a = _start(vae, 3, noise_mode=mode, light_path=[[0, angle]])
        gl, b = _start(vae, 3, noise_mode=mode, init_latent=side)
        assert gp.schedule == gl.schedule == (4, 2, 2) and a.dtype == H16 and tuple(a.shape) == (3, 4, 8, 8)
        assert torch.equal(a, b), (angle, side)
        assert torch.equal(torch.randn(4, generator=gp.rng_dev, device="cuda"), torch.randn(4, generator=gl.rng_dev, device="cuda"))
    _, c = _start(vae, 3, noise_mode=mode, light_path=[[0, 37.5]])
    assert not torch.equal(a, c) and torch.isfinite(c.float()).all()


@pytest.mark.parametrize("mode", ["same", "vanilla"])
def test_sweep_gives_every_frame_the_start_of_its_own_angle(L, vae, mode):
    g, sweep = _start(vae, 3, noise_mode=mode, light_path=[[0, 0], [1, 180]])
    assert g.light_angles == [0.0, 90.0, 180.0] and tuple(sweep.shape) == (3, 4, 8, 8)
    for i, a in enumerate(g.light_angles):
        _, alone = _start(vae, 3, noise_mode=mode, light_path=[[0, a]])
        assert torch.equal(sweep[i], alone[i]), (i, a)
    _, top = _start(vae, 3, noise_mode=mode, init_latent="top")
    assert torch.equal(sweep[1], top[1])
    assert not torch.equal(sweep[0], sweep[1]) and not torch.equal(sweep[1], sweep[2]) and not torch.equal(sweep[0], sweep[2])
    # general angles: five frames, 0 / 56.25 / 112.5 / 168.75 / 225 -- one axis-aligned image and four from the kernel, encoded in batches of two
    g5, s5 = _start(vae, 5, noise_mode=mode, light_path=[[0, 0], [1, 225]])
    assert g5.light_angles == [0.0, 56.25, 112.5, 168.75, 225.0]
    for i in (1, 4):
        _, alone = _start(vae, 5, noise_mode=mode, light_path=[[0, g5.light_angles[i]]])
        assert torch.equal(s5[i], alone[i]), i


def test_two_rank_split_builds_the_one_rank_start(L, vae):
    from tc_light_amd.parallel import Dist
    n, path = 5, [[0, 0], [0.5, 135], [1, 405]]                 # blocks of 3 and 2 frames; the second rank's positions are 0.75 and 1
    g, whole = _start(vae, n, noise_mode="vanilla", light_path=path)
    assert g.light_angles == [0.0, 67.5, 135.0, 270.0, 405.0]
    parts, angles = [], []
    for rank in range(2):
        d = Dist(rank, 2)
        lo, hi = d.range(n)
        gr, part = _start(vae, hi - lo, dist=d, n_total=n, noise_mode="vanilla", light_path=path)
        parts.append(part)
        angles += gr.light_angles
    assert [p.shape[0] for p in parts] == [3, 2] and angles == g.light_angles and torch.equal(torch.cat(parts), whole)


# ---------------------------------------------------------------------------------------------------------------- the whole Generator
def _run(unet, vae, n=3, **over):
    from tc_light_amd.generate import Generator
    from tc_light_amd.vidtome import VidToMe
    unet.tome = VidToMe("cuda", seed=5)                           # fresh draws: every run sees the same random frames / coins
    cfg = dict(n_timesteps=2, init_strength=0.5, alpha_t=0.0, chunk_size=4, seed=31, noise_mode="same", apply_opt=False, fbc_matting=False)
    cfg.update(over)
    g = Generator(unet, vae, cfg)
    seen = []
    sample = g.ddim_sample

    def recording(x, conds, conds_t, concat_conds, **kw):
        seen.append((x.clone(), concat_conds))
        return sample(x, conds, conds_t, concat_conds, **kw)
    g.ddim_sample = recording
    gen = torch.Generator().manual_seed(9)
    frames = torch.rand(n, 3, 64, 64, generator=gen).cuda()
    conds = torch.randn(2, 77, 768, generator=gen).half().cuda()
    out, info = g(frames, conds, conds, None, None, None)
    torch.cuda.synchronize()
    del g.ddim_sample                                               # the recorder held g through the bound method: no cycle is left behind
    assert len(seen) == 1 and torch.isfinite(out).all() and tuple(out.shape) == (n, 3, 64, 64)
    return g, out, info, seen[0]


def test_fc_constant_path_is_the_init_latent_run(L, unet8, vae):
    gp, a, ia, (xa, _) = _run(unet8, vae, light_path=[[0, 0]])
    gl, b, ib, (xb, _) = _run(unet8, vae, init_latent="left")
    assert torch.equal(xa, xb) and torch.equal(a, b)                # the start latents, then the relit frames
    assert (ia["scheduler_steps"], ia["steps_executed"]) == (ib["scheduler_steps"], ib["steps_executed"]) == (4, 2)
    assert ia["init_latent"] == "none" and ib["init_latent"] == "left"
    gs, c, _, (xc, _) = _run(unet8, vae, light_path=[[0, 0], [1, 180]])
    assert gs.light_angles == [0.0, 90.0, 180.0] and torch.equal(xc[0], xa[0]) and not torch.equal(xc[1], xa[1]) and not torch.equal(c, a)


def test_fbc_constant_path_is_the_bg_source_run_and_a_sweep_runs(L, unet12, vae):
    gp, a, _, (xa, (fga, bga)) = _run(unet12, vae, iclight_model="fbc", light_path=[[0, 180]])
    gr, b, _, (xb, (fgb, bgb)) = _run(unet12, vae, iclight_model="fbc", bg_source="right")
    assert tuple(bga.shape) == (1, 4, 8, 8) and torch.equal(gp.bg_frames, gr.bg_frames) and torch.equal(bga, bgb) and torch.equal(fga, fgb)
    assert torch.equal(xa, xb) and torch.equal(a, b)
    gs, c, info, (xc, (fgc, bgc)) = _run(unet12, vae, iclight_model="fbc", light_path=[[0, 180], [1, 300]])
    assert gs.light_angles == [180.0, 240.0, 300.0] and info["iclight_model"] == "fbc" and gs.schedule == (2, 0, 2)
    assert tuple(bgc.shape) == (3, 4, 8, 8) and bgc.dtype == H16 and torch.equal(fgc, fga) and torch.equal(xc, xa)      # the noise start is untouched
    assert tuple(gs.bg_frames.shape) == (3, 3, 64, 64)             # three distinct ramps
    for i, angle in enumerate(gs.light_angles):
        imgs, index = gs.light_ramps([angle], 64, 64, 224, 32)
        assert index == [0] and torch.equal(imgs[0], gs.bg_frames[i])
        assert torch.equal(bgc[i:i + 1], vae.encode(imgs)), i       # each frame's background latent: the encode of its ramp alone
    assert torch.equal(bgc[0:1], bga) and not torch.equal(c, a)
    (cc, ss), = R.dirs([240.0])
    assert np.array_equal(gs.bg_frames[1].cpu().numpy().view(np.uint32), R.ramp_image(cc, ss, 64, 64, 224, 32).view(np.uint32))
    # a sweep that comes back to where it began: 180, 270, 360 + 180 -> two distinct ramps for three frames, gathered
    g2, _, _, (_, (_, bg2)) = _run(unet12, vae, iclight_model="fbc", light_path=[[0, 180], [1, 540]])
    assert g2.light_angles == [180.0, 360.0, 540.0] and tuple(g2.bg_frames.shape) == (2, 3, 64, 64) and g2.bg_index.tolist() == [0, 1, 0]
    assert tuple(bg2.shape) == (3, 4, 8, 8) and torch.equal(bg2[0], bg2[2]) and not torch.equal(bg2[0], bg2[1])


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_with_light_sweep(L, tmp_path):
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(__file__))
    import synth
    import run
    d = synth.video_clip(3, 64, 64, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{rgb_path: {vid}, height: 64, width: 64}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 2
  alpha_t: 0.01
  frame_range: [0, 3, 1]
post_opt: {{apply_opt: false}}
models: {{allow_random: true}}
""")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:                                                            # one run: loading the stand-in models is most of its time
        run.main(["--config", str(cfg), "--light_sweep", "-90", "405", "--strength", "0.5"])
    finally:
        os.chdir(cwd)
    outs = [os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "work") for f in fs if f == "output.npy"]
    assert len(outs) == 1
    out = np.load(outs[0])
    assert out.shape == (3, 64, 64, 3) and out.dtype == np.uint8 and out.std() > 0
    gs = yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))["generation"]
    assert gs["light_path"] == [[0.0, -90.0], [1.0, 405.0]] and (gs["light_angle_first"], gs["light_angle_last"]) == (-90.0, 405.0)
    assert (gs["init_latent"], gs["init_strength"], gs["scheduler_steps"], gs["steps_executed"]) == ("none", 0.5, 4, 2)
