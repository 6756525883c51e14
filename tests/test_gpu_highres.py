"""GPU: the highres pass (generation.highres_scale / highres_denoise; IC-Light's process(), gradio_demo_iclight.py:301-334; csrc/resize.hip).
  * tcl_resize_lanczos_u8 against tests/highres_refs.py (pinned to PIL itself in tests/test_highres_refs_cpu.py), byte for byte, on every case of
    the table with N = 3, a sentinel-filled output and a guard row; its refusals;
  * tcl_frames_to_u8 on k/255 and one ulp either side, values outside [0, 1] and -0.0, against the restatement, exactly;
  * the upscale stage of the Generator: u8 planes = refs(quantise -> resize) of the decoded frames, x0 = vae.encode(u8/254) bit for bit;
  * the whole Generator at 64x64 -> 128x128, 4 frames, n_timesteps 4: shape, finiteness, run-to-run bits, the first pass untouched, the
    second schedule, and the relation "a weaker second denoise stays closer to the upscaled first pass".  (img2img_schedule(4, 0.25) is (16, 12, 4):
    the last four of sixteen steps, the low-noise quarter of the schedule -- not one step; (4, 1.0) is the whole schedule from pure noise level.)
  * run.py end to end with the pass on: the result, output_gt and the producers at the final size, the config.yaml keys, no flow cache.
Seeded random weights everywhere: parity and plumbing, not image quality."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import highres_refs as R

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


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


@pytest.fixture(scope="module")
def unet(L):
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    return UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(), seed=1), "cuda", VidToMe("cuda", seed=5))


def st():
    return torch.cuda.current_stream().cuda_stream


def _stub_unet():
    return SimpleNamespace(dev=torch.device("cuda"), tome=SimpleNamespace(args={}))


def _table(L, n_in, n_out):
    if n_in == n_out:
        return 0
    t = torch.empty(L.tcl_resize_lanczos_table_ints(n_in, n_out), dtype=torch.int32)
    L.tcl_resize_lanczos_table(n_in, n_out, t)
    return t.cuda()


# ---------------------------------------------------------------------------------------------------------------- kernels, bit for bit
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}->{c[1][0]}x{c[1][1]}")
def test_resize_bits(L, case):
    (h, w), (ho, wo) = case
    N = 3
    tx, ty = _table(L, w, wo), _table(L, h, ho)
    for kind in R.CONTENTS:
        img = R.content(kind, N, h, w, seed=h * 1000 + w)
        out = torch.full((N * ho * wo * 3 + wo * 3,), SENTINEL, dtype=torch.uint8, device="cuda")      # one guard row behind the frames
        L.tcl_resize_lanczos_u8(torch.from_numpy(img).cuda(), out, N, h, w, ho, wo, tx, ty, st())
        got = out.cpu().numpy()
        want = R.resize_lanczos(img, ho, wo)
        assert (got[N * ho * wo * 3:] == SENTINEL).all(), kind
        diff = got[:N * ho * wo * 3].reshape(N, ho, wo, 3) != want
        assert not diff.any(), f"{kind}: {int(diff.sum())} bytes differ, first at {np.argwhere(diff)[0].tolist()}"


def test_resize_odd_output_width_and_copy(L):
    """An output row that is no multiple of 4 bytes (byte stores), a partial tile in both directions, and the no-op size (a copy)."""
    img = R.content("random", 2, 50, 37, seed=5)
    x = torch.from_numpy(img).cuda()
    for ho, wo in ((75, 51), (50, 37), (50, 45), (67, 37), (75, 52)):
        off = 1 if (ho, wo) == (75, 52) else 0                     # rows of whole dwords behind an unaligned destination: byte stores too
        out = torch.full((off + 2 * ho * wo * 3 + wo * 3,), SENTINEL, dtype=torch.uint8, device="cuda")
        L.tcl_resize_lanczos_u8(x, out[off:], 2, 50, 37, ho, wo, _table(L, 37, wo), _table(L, 50, ho), st())
        got = out.cpu().numpy()
        assert np.array_equal(got[off:off + 2 * ho * wo * 3].reshape(2, ho, wo, 3), R.resize_lanczos(img, ho, wo)), (ho, wo)
        assert (got[off + 2 * ho * wo * 3:] == SENTINEL).all() and (got[:off] == SENTINEL).all()


def test_resize_refuses_bad_arguments(L):
    x = torch.zeros(3 * 64 * 64 * 3, dtype=torch.uint8, device="cuda")
    out = torch.zeros(3 * 128 * 128 * 3, dtype=torch.uint8, device="cuda")
    t = _table(L, 64, 128)
    bad = [(0, out, 1, 64, 64, 128, 128, t, t), (x, 0, 1, 64, 64, 128, 128, t, t),           # null pointers
           (x, out, 1, 64, 64, 128, 128, 0, t), (x, out, 1, 64, 64, 128, 128, t, 0),         # a resampled axis without its table
           (x, out, 0, 64, 64, 128, 128, t, t), (x, out, 1, 0, 64, 128, 128, t, t), (x, out, 1, 64, 64, 128, -128, t, t),
           (x, out, 1, 16, 64, 65, 128, t, t),                                              # ratio below 0.25
           (x, out, 1, 64, 129, 128, 64, t, t),                                             # ratio above 2
           (x, out, 3, 64, 64, 128 * 128, 128 * 128, t, t),                                 # ratio, and 3 N Ho Wo >= 2^31
           (x, out, 2731, 256, 512, 512, 512, t, t)]                                        # 3 * 2731 * 512 * 512 >= 2^31 with legal ratios
    for args in bad:
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_resize_lanczos_u8(*args, st())
    assert L.tcl_resize_lanczos_table_ints(16, 65) == 0 and L.tcl_resize_lanczos_table_ints(129, 64) == 0
    torch.cuda.synchronize()
    assert not out.any().item()


@pytest.mark.parametrize("H,W", [(2, 389), (4, 389), (1, 1)])
def test_quantise_bits(L, H, W):
    """H * W % 4 != 0 takes the one-pixel path, == 0 the 16-byte one; every probe value lands in every channel."""
    v = R.quantise_probes()
    assert v.size == 778
    p = np.stack([np.stack([np.resize(np.roll(v, 7 * c + 131 * n), H * W).reshape(H, W) for c in range(3)]) for n in range(2)]).astype(np.float32)
    out = torch.full((2 * H * W * 3 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    L.tcl_frames_to_u8(torch.from_numpy(p).cuda(), out, 2, H, W, st())
    got = out.cpu().numpy()
    assert np.array_equal(got[:2 * H * W * 3].reshape(2, H, W, 3), R.frames_to_u8(p)) and (got[2 * H * W * 3:] == SENTINEL).all()
    back = torch.empty(2, 3, H, W, device="cuda")
    L.tcl_u8_to_frames_f32(out, back, 2, H, W, 254.0, st())
    want = R.frames_to_u8(p).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(254)      # numpy: one IEEE division (torch multiplies by 1/254)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for args in ((0, out, 2, H, W), (torch.from_numpy(p).cuda(), 0, 2, H, W), (torch.from_numpy(p).cuda(), out, 0, H, W),
                 (torch.from_numpy(p).cuda(), out, 2, 1 << 15, 1 << 15)):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_frames_to_u8(*args, st())


# ---------------------------------------------------------------------------------------------------------------- the upscale stage
def test_upscale_stage(L, vae):
    from tc_light_amd.generate import Generator
    g = Generator(_stub_unet(), vae, dict(highres_scale=2.0, max_tokens_per_pass=1 << 20))
    z = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(4)).half().cuda()
    decoded = vae.decode_latents_batch(z, 2)
    assert tuple(decoded.shape) == (4, 3, 64, 64)
    up, x0 = g.highres_upscale(decoded)
    want = R.resize_lanczos(R.frames_to_u8(decoded.cpu().numpy()), 128, 128)
    assert up.dtype == torch.uint8 and np.array_equal(up.cpu().numpy(), want)
    assert len(np.unique(want)) > 16                                  # the random decoder fills the range: not a constant image
    img = torch.from_numpy(np.ascontiguousarray(want.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(254)).cuda()      # one IEEE division
    ref = torch.cat([vae.encode(b.contiguous()) for b in img.split(g.batch_size)])
    assert tuple(x0.shape) == (4, 4, 16, 16) and x0.dtype == torch.float16 and torch.equal(x0, ref)


# ---------------------------------------------------------------------------------------------------------------- the whole Generator
def _run(unet, vae, mode, alpha_t, **over):
    from tc_light_amd.generate import Generator
    from tc_light_amd.vidtome import VidToMe
    unet.tome = VidToMe("cuda", seed=5)                               # fresh draws: every run sees the same random frames / coins
    cfg = dict(n_timesteps=4, alpha_t=alpha_t, final_factor_t=0.5, win_size_t=4, chunk_size=4, seed=31, noise_mode=mode, apply_opt=False)
    cfg.update(over)
    g = Generator(unet, vae, cfg)
    gen = torch.Generator().manual_seed(9)
    frames = torch.rand(4, 3, 64, 64, generator=gen).cuda()
    frames_hr = torch.rand(4, 3, 128, 128, generator=gen).cuda()
    conds = torch.randn(2, 77, 768, generator=gen).half().cuda()
    conds_t = torch.randn(2, 77, 768, generator=gen).half().cuda()
    out, info = g(frames, conds, conds_t, None, None, None, frames_hr=frames_hr if g.highres else None)
    torch.cuda.synchronize()
    return g, out, info


@pytest.mark.parametrize("mode,alpha_t", [("same", 0.0), ("vanilla", 0.0), ("vanilla", 0.3)])
def test_generator_highres(L, unet, vae, mode, alpha_t):
    from tc_light_amd import hostlogic as HL
    g_off, out_off, info_off = _run(unet, vae, mode, alpha_t)
    assert tuple(out_off.shape) == (4, 3, 64, 64) and "highres_size" not in info_off
    ga, a, ia = _run(unet, vae, mode, alpha_t, highres_scale=2.0, highres_denoise=0.25)
    gb, b, ib = _run(unet, vae, mode, alpha_t, highres_scale=2.0, highres_denoise=0.25)
    gc, c, ic = _run(unet, vae, mode, alpha_t, highres_scale=2.0, highres_denoise=1.0)
    for out in (a, b, c):
        assert tuple(out.shape) == (4, 3, 128, 128) and out.dtype == torch.float32 and torch.isfinite(out).all()
    assert torch.equal(a, b)                                           # two runs, the same bits
    for g in (ga, gb, gc):                                             # the first pass is what it is without the second
        assert torch.equal(g.latents, g_off.latents) and tuple(g.latents.shape) == (4, 4, 8, 8)
    assert torch.equal(ga.upscaled_u8, gc.upscaled_u8)
    assert ia["highres_size"] == [128, 128] and (ia["scheduler_steps"], ia["steps_executed"]) == (4, 4)
    assert (ia["highres_scheduler_steps"], ia["highres_steps_executed"]) == HL.img2img_schedule(4, 0.25)[::2] == (16, 4)
    assert (ic["highres_scheduler_steps"], ic["highres_steps_executed"]) == HL.img2img_schedule(4, 1.0)[::2] == (4, 4)
    assert ia["timing"]["highres"] > 0 and "highres" not in info_off["timing"]
    up = ga.upscaled_u8.permute(0, 3, 1, 2).float() / 255
    near, far = (a - up).abs().mean().item(), (c - up).abs().mean().item()
    print(f"[highres] {mode} alpha_t {alpha_t}: mean |out - upscaled first pass| = {near:.4f} at denoise 0.25, {far:.4f} at 1.0")
    assert near < far                                                  # fails if x0 never reaches the start latents


def test_generator_refuses_background_and_missing_frames(L, unet, vae):
    from tc_light_amd.generate import Generator
    g = Generator(unet, vae, dict(n_timesteps=1, highres_scale=2.0, apply_opt=False))
    fr = torch.zeros(2, 3, 64, 64, device="cuda")
    cd = torch.zeros(2, 77, 768, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="background_cond"):
        g(fr, cd, cd, None, None, None, background=fr[:1], frames_hr=torch.zeros(2, 3, 128, 128, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_with_highres(L, tmp_path):
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(__file__))
    import synth
    import run
    d = synth.video_clip(4, 128, 192, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{rgb_path: {vid}, height: 128, width: 192}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 1
  alpha_t: 0.01
  frame_range: [0, 4, 1]
post_opt: {{epochs_exposure: 1, epochs: 1, batch_size: 4}}
models: {{allow_random: true}}
""")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        run.main(["--config", str(cfg), "--highres_scale", "1.5", "--highres_denoise", "0.5"])
    finally:
        os.chdir(cwd)
    outs = [os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "work") for f in fs if f == "output.npy"]
    assert len(outs) == 1
    out = np.load(outs[0])
    assert out.shape == (4, 192, 256, 3) and out.dtype == np.uint8          # 128 * 1.5 = 192; 192 * 1.5 / 64 = 4.5 rounds half to even: 256
    odir = os.path.dirname(outs[0])
    gts = [f for f in os.listdir(odir) if f.startswith("output_gt")]
    assert gts
    from tc_light_amd.dataparser import read_frames
    gt = read_frames(os.path.join(odir, gts[0]))
    assert tuple(gt.shape) == (4, 3, 192, 256)
    saved = yaml.safe_load(open(os.path.join(odir, "config.yaml")))["generation"]
    assert saved["highres_scale"] == 1.5 and saved["highres_denoise"] == 0.5 and saved["highres_size"] == [192, 256]
    assert (saved["scheduler_steps"], saved["steps_executed"]) == (1, 1)
    assert (saved["highres_scheduler_steps"], saved["highres_steps_executed"]) == (2, 1)
    assert os.path.exists(os.path.join(odir, "loss_exposure.npy")) and os.path.exists(os.path.join(odir, "loss_unique_tensor.npy"))
    assert not [f for f in os.listdir(tmp_path) if "flow" in f]               # the cache belongs to the working size: not written
