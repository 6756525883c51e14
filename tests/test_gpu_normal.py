"""GPU: generation.normal (IC-Light's "Compute Normal", the background demo's process_normal, on the fbc model).
  * tcl_matte_grey_sigma_f32: sigma = 0 is tcl_matte_grey_f32 bit for bit, sigma = 16 the integers of normal_refs.matte_q, at 5x7 (scalar path)
    and 64x64 (16 B path);
  * tcl_fbc_normal: the exact cases; the general case against float64 within multiples of D (what float32 rounding alone costs on these inputs,
    tests/normal_refs.py, tests/test_normal_refs_cpu.py), aligned and misaligned, every output between sentinel guards; the refusals;
  * Generator.normals on tiny seeded fbc fixtures: every direction is the plain run with that bg_source, bit for bit; run.py --normal end to end.
Seeded random weights everywhere: parity and plumbing, not image quality."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import normal_refs as R

pytestmark = pytest.mark.gpu
H16 = torch.float16
F32 = np.float32
GUARD = 0x5A


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


@pytest.fixture(scope="module")
def unet(L):
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    return UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(in_channels=12), seed=1), "cuda", VidToMe("cuda", seed=5))


@pytest.fixture(scope="module")
def vae(L):
    from tc_light_amd import sd15
    from tc_light_amd.vae import VAEEngine
    return VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")


@pytest.fixture(scope="module")
def rmbg(L):
    import warnings
    from tc_light_amd.model_utils import load_rmbg_state
    from tc_light_amd.rmbg import RMBGEngine
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return RMBGEngine(load_rmbg_state(None, allow=True), "cuda")


def st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- the matte with sigma
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_matte_sigma(L, H, W):
    n = R.N_FRAMES
    k = np.random.default_rng(H * 100 + W).integers(0, 256, size=(n, 3, H, W))
    f = (k.astype(F32) / F32(255)).astype(F32)                             # inputs k/255
    a = np.random.default_rng(H + W).random((n, 1, H, W), dtype=F32)
    a[0, 0].reshape(-1)[:6] = [0.0, 1.0, np.nan, 0.5, 1.0, 0.0]
    a[1, 0, -1, -3:] = [0.0, np.nan, 1.0]
    fd, ad = torch.from_numpy(f).cuda(), torch.from_numpy(a).cuda()
    size = n * 3 * H * W

    def run(fn, *extra):
        buf = torch.full((size + 4,), float("nan"), device="cuda")
        fn(fd, ad, buf, n, H, W, *extra, st())
        got = buf.cpu().numpy()
        assert np.isnan(got[size:]).all()
        return got[:size].reshape(n, 3, H, W)
    plain = run(L.tcl_matte_grey_f32)
    assert np.array_equal(run(L.tcl_matte_grey_sigma_f32, 0.0).view(np.uint32), plain.view(np.uint32))      # sigma 0: bit for bit
    got = run(L.tcl_matte_grey_sigma_f32, 16.0)
    q = R.matte_q(f, a, 16.0)
    assert q.shape == (n, 3, H, W) and len(np.unique(q)) > 16 and not np.array_equal(q, R.matte_q(f, a, 0.0))
    assert np.array_equal(got.view(np.uint32), (q.astype(F32) / F32(254)).view(np.uint32))
    assert np.array_equal(np.rint(F32(254) * got).astype(np.int64), q)
    od = torch.full((size,), 7.0, device="cuda")
    for args in ((0, ad, od, n, H, W, 16.0), (fd, 0, od, n, H, W, 16.0), (fd, ad, 0, n, H, W, 16.0), (fd, ad, od, 0, H, W, 16.0),
                 (fd, ad, od, n, 0, W, 16.0), (fd, ad, od, n, H, -1, 16.0), (fd, ad, od, n, H, W, float("nan"))):
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_matte_grey_sigma_f32(*args, st())
    assert (od == 7.0).all()                                               # a refusal writes nothing


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _guarded(nbytes, off):
    """A byte buffer filled with GUARD and the view of `nbytes` bytes at offset 64 + off inside it (the allocation is 256 B aligned)."""
    buf = torch.full((64 + off + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[64 + off:64 + off + nbytes]


def _intact(buf, nbytes, off):
    b = buf.cpu()
    return bool((b[:64 + off] == GUARD).all() and (b[64 + off + nbytes:] == GUARD).all())


def _at(x, off):
    """A device copy of the f32 array whose first element sits `off` bytes past a 256 B boundary."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.empty(t.numel() * 4 + 64, dtype=torch.uint8, device="cuda")
    v = buf[off:off + t.numel() * 4].view(torch.float32).view(t.shape)
    v.copy_(t)
    return v


def run_kernel(L, rel, alpha, off_in=0, off_u8=0, off_f32=0, want_f32=True, want_amb=True):
    n, _, H, W = rel[0].shape
    srcs = [_at(x, off_in) for x in rel]
    a = 0 if alpha is None else _at(alpha, off_in)
    bu, vu = _guarded(n * H * W * 3, off_u8)
    bf, vf = _guarded(n * 3 * H * W * 4, off_f32)
    ba, va = _guarded(n * 3 * H * W * 4, off_f32)
    L.tcl_fbc_normal(*srcs, a, vu, vf if want_f32 else 0, va if want_amb else 0, n, H, W, st())
    torch.cuda.synchronize()
    assert _intact(bu, n * H * W * 3, off_u8)
    assert _intact(bf, n * 3 * H * W * 4 if want_f32 else 0, off_f32) and _intact(ba, n * 3 * H * W * 4 if want_amb else 0, off_f32)
    return (vu.cpu().numpy().reshape(n, H, W, 3), vf.view(torch.float32).cpu().numpy().reshape(n, 3, H, W) if want_f32 else None,
            va.view(torch.float32).cpu().numpy().reshape(n, 3, H, W) if want_amb else None)


FLAT = np.array([127, 127, 255], dtype=np.uint8)


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_normal_exact_cases(L, H, W):
    n = R.N_FRAMES
    g = np.random.default_rng(H + 3 * W)
    x = g.random((n, 3, H, W), dtype=F32)
    a = g.random((n, 1, H, W), dtype=F32)
    for same in (x, np.zeros_like(x)):                                     # four identical inputs, all-zero frames included
        for alpha in (a, None):
            u8, f32, amb = run_kernel(L, [same] * 4, alpha)
            assert (u8 == FLAT).all()
            assert (f32[:, :2] == 0).all() and np.abs(f32[:, 2] - 1).max() <= 2.0 ** -23
    rel, _ = R.kernel_inputs(H, W)
    u8, f32, _ = run_kernel(L, rel, np.zeros_like(a))                       # alpha 0: flat whatever the inputs
    assert (u8 == FLAT).all() and (f32[:, :2] == 0).all() and (f32[:, 2] == 1).all()
    none, one = run_kernel(L, rel, None), run_kernel(L, rel, np.ones_like(a))      # alpha NULL is alpha 1
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(none, one))
    assert not (none[0] == FLAT).all()


@pytest.mark.parametrize("offs", [(0, 0, 0), (4, 0, 0), (0, 1, 0), (0, 0, 4), (8, 3, 12)], ids=["aligned", "in+4", "u8+1", "f32+4", "all_off"])
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_normal_general(L, H, W, offs):
    """5x7 always takes the scalar path (H*W % 4 != 0); 64x64 takes the 16 B path when aligned and the scalar path with any pointer off."""
    cases, D = R.parity()
    c = cases[(H, W)]
    u8, f32, amb = run_kernel(L, c["rel"], c["alpha"], *offs)
    assert np.isfinite(f32).all() and np.isfinite(amb).all()
    dev = float(np.abs(f32.astype(np.float64) - c["f64"]["normal"]).max())
    print(f"[normal] {H}x{W} offsets {offs}: max|normal_f32 - f64| = {dev:.3e} (D = {D:.3e}, bound 4 D = {4 * D:.3e})")
    assert np.array_equal(amb.view(np.uint32), c["f32"]["ambient"].view(np.uint32))                 # bit-exact against f32 numpy
    y = c["f64"]["y"]
    want = np.trunc(y).astype(np.int64)
    diff = u8.astype(np.int64) - want
    loose = np.abs(y - np.rint(y)) <= 512 * D                               # per value: the float64 value lies within 512 D of an integer
    n_loose = int(loose.any(axis=-1).sum())
    print(f"[normal] {H}x{W} offsets {offs}: {int((diff != 0).sum())} u8 values differ from the float64 truncation; {n_loose} of {loose[..., 0].size} "
          f"pixels are within 512 D of an integer")
    assert dev <= 4 * D
    assert (diff[~loose] == 0).all() and (np.abs(diff[loose]) <= 1).all()
    assert len(np.unique(u8)) > 32
    # the optional outputs change nothing in the others
    u8b, _, ambb = run_kernel(L, c["rel"], c["alpha"], *offs, want_f32=False)
    u8c, f32c, _ = run_kernel(L, c["rel"], c["alpha"], *offs, want_amb=False)
    assert np.array_equal(u8b, u8) and np.array_equal(u8c, u8) and np.array_equal(ambb.view(np.uint32), amb.view(np.uint32))
    assert np.array_equal(f32c.view(np.uint32), f32.view(np.uint32))


def test_normal_excepted_pixels_are_few(L):
    """Over all the test inputs at most 1 % of the pixels may use the +-1 allowance."""
    cases, D = R.parity()
    near = sum(int(R.near_integer(c["f64"]["y"], 512 * D).sum()) for c in cases.values())
    total = sum(c["f64"]["y"][..., 0].size for c in cases.values())
    assert near <= 0.01 * total, (near, total)


def test_normal_refusals(L):
    n, H, W = 2, 5, 7
    rel, alpha = R.kernel_inputs(H, W)
    srcs = [torch.from_numpy(x).cuda() for x in rel]
    a = torch.from_numpy(alpha).cuda()
    u8 = torch.full((n, H, W, 3), GUARD, dtype=torch.uint8, device="cuda")
    f32 = torch.full((n, 3, H, W), 7.0, device="cuda")
    amb = torch.full((n, 3, H, W), 7.0, device="cuda")
    good = [*srcs, a, u8, f32, amb, n, H, W]
    for pos in (0, 1, 2, 3, 5):                                            # the four relights and normal_u8 are required
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_fbc_normal(*[0 if k == pos else v for k, v in enumerate(good)], st())
    for pos, bad in ((8, 0), (8, -1), (9, 0), (10, 0), (10, -3)):            # non-positive sizes
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_fbc_normal(*[bad if k == pos else v for k, v in enumerate(good)], st())
    for nn, hh, ww in ((1, 26755, 26755), (2 ** 20, 1, 683), (3, 16384, 43691)):      # 3 n H W >= 2^31 (the first: 3 H W just past it)
        assert 3 * nn * hh * ww >= 2 ** 31
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_fbc_normal(*good[:8], nn, hh, ww, st())
    torch.cuda.synchronize()
    assert (u8 == GUARD).all() and (f32 == 7.0).all() and (amb == 7.0).all()      # a refusal writes nothing
    L.tcl_fbc_normal(*good, st())
    torch.cuda.synchronize()
    assert not (u8 == GUARD).all()


# ---------------------------------------------------------------------------------------------------------------- the Generator
def _inputs():
    gen = torch.Generator().manual_seed(9)
    frames = torch.rand(2, 3, 64, 64, generator=gen).cuda()
    conds = torch.randn(2, 77, 768, generator=gen).half().cuda()
    return frames, conds


def _gen(unet, vae, rmbg=None, **over):
    from tc_light_amd.generate import Generator
    from tc_light_amd.vidtome import VidToMe
    unet.tome = VidToMe("cuda", seed=5)                                    # fresh draws: every run sees the same random frames / coins
    cfg = dict(n_timesteps=1, alpha_t=0.0, chunk_size=4, seed=31, noise_mode="same", apply_opt=False, iclight_model="fbc", fbc_matting=False)
    cfg.update(over)
    return Generator(unet, vae, cfg, rmbg=rmbg)


@pytest.fixture(scope="module")
def normals_run(unet, vae):
    frames, conds = _inputs()
    g = _gen(unet, vae, normal=True)
    out = g.normals(frames, conds, conds)
    torch.cuda.synchronize()
    return g, out


def test_generator_normals(L, unet, vae, normals_run):
    g, (nrm, amb, relit, info) = normals_run
    frames, conds = _inputs()
    assert tuple(nrm.shape) == (2, 64, 64, 3) and nrm.dtype == torch.uint8 and tuple(amb.shape) == (2, 3, 64, 64) and amb.dtype == torch.float32
    assert tuple(relit) == ("left", "right", "bottom", "top") and all(tuple(r.shape) == (2, 3, 64, 64) for r in relit.values())
    assert set(info["denoise_per_direction"]) == set(relit) and info["total_time"] > 0 and info["sec_per_frame"] == info["total_time"] / 2
    assert info["apply_opt"] is False and torch.equal(g.fg_frames, frames)                          # fbc_matting false: the frames as they are
    assert not torch.equal(relit["left"], relit["right"]) and not torch.equal(relit["top"], relit["bottom"])
    for side in ("left", "top"):                                           # the first and the last direction: the plain run with that bg_source
        plain, _ = _gen(unet, vae, bg_source=side)(frames, conds, conds, None, None, None)
        torch.cuda.synchronize()
        assert torch.equal(relit[side], plain), side
    # the normal is the kernel applied to the four returned relights (alpha NULL)
    want = torch.empty_like(nrm)
    want_amb = torch.empty_like(amb)
    L.tcl_fbc_normal(*(relit[s].contiguous() for s in R.SIDES), 0, want, 0, want_amb, 2, 64, 64, st())
    torch.cuda.synchronize()
    assert torch.equal(nrm, want) and torch.equal(amb, want_amb) and len(torch.unique(nrm)) > 8
    # a second call: the same bits
    nrm2, amb2, relit2, _ = _gen(unet, vae, normal=True).normals(frames, conds, conds)
    torch.cuda.synchronize()
    assert torch.equal(nrm, nrm2) and torch.equal(amb, amb2) and all(torch.equal(relit[s], relit2[s]) for s in relit)


def test_generator_normals_with_matting(L, unet, vae, rmbg, normals_run):
    """fbc_matting: true -- the foreground is the sigma-16 matte of this run's frames and alpha, and that alpha reaches the kernel."""
    frames, conds = _inputs()
    g = _gen(unet, vae, rmbg, normal=True, fbc_matting=True)
    nrm, amb, relit, info = g.normals(frames, conds, conds)
    torch.cuda.synchronize()
    alpha = rmbg.estimate_alpha(frames, 2).float().contiguous()
    assert tuple(alpha.shape) == (2, 1, 64, 64)
    q = R.matte_q(frames.cpu().numpy(), alpha.cpu().numpy(), 16.0)
    assert np.array_equal(g.fg_frames.cpu().numpy().view(np.uint32), (q.astype(F32) / F32(254)).view(np.uint32))
    assert not np.array_equal(q, R.matte_q(frames.cpu().numpy(), alpha.cpu().numpy(), 0.0))          # the offset is live
    assert torch.equal(g.frames, frames) and not torch.equal(g.fg_frames, frames)
    want, want_amb = torch.empty_like(nrm), torch.empty_like(amb)
    L.tcl_fbc_normal(*(relit[s].contiguous() for s in R.SIDES), alpha, want, 0, want_amb, 2, 64, 64, st())
    torch.cuda.synchronize()
    assert torch.equal(nrm, want) and torch.equal(amb, want_amb)
    # the matted foreground is a live condition: the relights differ from the run without matting
    assert not torch.equal(relit["left"], normals_run[1][2]["left"])
    with pytest.raises(RuntimeError, match="fbc_matting"):                 # matting on and no engine: an error, not a silent pass-through
        _gen(unet, vae, None, normal=True, fbc_matting=True).normals(frames, conds, conds)


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_normal(L, tmp_path):
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
  prompt: {{edit: "soft light"}}
  n_timesteps: 1
  alpha_t: 0.0
  frame_range: [0, 3, 1]
  iclight_model: fbc
  bg_source: upload
models: {{allow_random: true}}
""")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        run.main(["--config", str(cfg), "--normal"])        # bg_source upload without a background_image_path: not consulted; apply_opt true in the base
    finally:
        os.chdir(cwd)
    dirs = [r for r, _, fs in os.walk(tmp_path / "work") if "normal.npy" in fs]
    assert len(dirs) == 1
    files = os.listdir(dirs[0])
    nrm = np.load(os.path.join(dirs[0], "normal.npy"))
    assert nrm.shape == (3, 64, 64, 3) and nrm.dtype == np.uint8 and len(np.unique(nrm)) > 8
    for side in R.SIDES:
        r = np.load(os.path.join(dirs[0], f"relit_{side}.npy"))
        assert r.shape == (3, 64, 64, 3) and r.dtype == np.uint8
    out = np.load(os.path.join(dirs[0], "output.npy"))                     # the ambient video
    assert out.shape == (3, 64, 64, 3) and out.dtype == np.uint8
    stems = {os.path.splitext(f)[0] for f in files}
    assert {"normal", "output", "output_gt", "config"} <= stems
    assert any(f in files for f in ("normal.mp4", "normal.avi")) and any(f in files for f in ("output.mp4", "output.avi"))
    saved = yaml.safe_load(open(os.path.join(dirs[0], "config.yaml")))
    assert saved["generation"]["normal"] is True and saved["post_opt"]["apply_opt"] is False
    assert saved["generation"]["iclight_model"] == "fbc" and set(saved["generation"]["normal_denoise_seconds"]) == set(R.SIDES)
    assert not any(f.startswith("loss_") for f in files)                   # no stage 1 / 2
