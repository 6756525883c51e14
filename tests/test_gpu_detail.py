"""generation.detail_transfer on the GPU: tcl_detail_transfer_f32 against the float64 reference and its derived per-element bound (tests/detail_refs.py)
on the case table -- overlapping reflections, the kernels' tile and row-segment sizes -1 / 0 / +1, two different frames, the largest radius at the smallest
legal height, masks with 0, 1 and fractions and none, both modes and both channel settings on every geometry -- the bit-for-bit identities, the refusals,
then the step inside the Generator (fc and fbc) and run.py --detail.  Outputs sit between sentinel guards."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import detail_refs as R

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0x7FC12345                                  # a NaN bit pattern no arithmetic here produces
GEOMS = sorted(R.geometries())


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape):
    """-> (buffer of int32 sentinels, f32 view of `shape` inside it with GUARD sentinels on both sides)."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float32).view(*shape)


def guards_kept(buf, n):
    return bool((buf[:GUARD] == SENT).all() and (buf[GUARD + n:] == SENT).all())


def call(L, S, Rl, mask, sigma, mode, channels, blend, change=None):
    """One direct call of the C entry on host arrays -> out on the host.  change: arguments replaced to provoke a refusal, which is raised again
    after the buffers were looked at."""
    from tc_light_amd import detail
    taps, r = detail.gaussian_taps(sigma)
    N, _, H, W = S.shape
    s, q = torch.from_numpy(S).cuda(), torch.from_numpy(Rl).cuda()
    m = 0 if mask is None else torch.from_numpy(mask).cuda()
    k = dict(src=s, relit=q, mask=m, N=N, H=H, W=W, taps=taps, n_taps=taps.numel(), radius=r, mode=detail.MODES.index(mode),
             luma=detail.CHANNELS.index(channels), blend=blend)
    buf, out = guarded(S.shape)
    k["out"] = out
    k.update({key: (s if isinstance(v, str) and v == "src" else v) for key, v in (change or {}).items()})      # "src": alias the source frames
    ws_bytes = max(L.tcl_detail_transfer_workspace_bytes(N, H, W, detail.MODES.index(mode), detail.CHANNELS.index(channels)), 4)
    wbuf, ws = guarded((ws_bytes // 4,))
    k.setdefault("ws", ws)
    k.setdefault("ws_bytes", ws_bytes)
    refused = None
    try:
        L.tcl_detail_transfer_f32(k["src"], k["relit"], k["mask"], k["out"], k["N"], k["H"], k["W"], k["taps"], k["n_taps"], k["radius"], k["mode"],
                                  k["luma"], k["blend"], k["ws"], k["ws_bytes"], st())
    except RuntimeError as e:
        refused = e
    torch.cuda.synchronize()
    assert guards_kept(buf, out.numel()) and guards_kept(wbuf, ws.numel()), "a guard next to the output or the workspace was written"
    assert torch.equal(s.cpu(), torch.from_numpy(S)) and torch.equal(q.cpu(), torch.from_numpy(Rl)), "an input was written"
    if refused is not None:                                      # a refused call writes nothing: output and workspace keep their fill
        assert bool((buf == SENT).all()) and bool((wbuf == SENT).all()), f"a refused call wrote something ({change})"
        raise refused
    return out.cpu().numpy()


@pytest.mark.parametrize("mode,channels", R.SETTINGS)
@pytest.mark.parametrize("name", GEOMS)
def test_kernel_within_bound_of_float64(L, name, mode, channels):
    c = R.case(name, mode, channels)
    got = call(L, c["S"], c["R"], c["mask"], c["sigma"], mode, channels, R.BLEND)
    err = np.abs(got.astype(np.float64) - c["ref"])
    worst = (err / np.maximum(c["bound"], 1e-300)).max()
    print(f"{name} {mode} {channels}: max |err| {err.max():.3e}, max err/bound {worst:.3f}, moved {(got != c['R']).mean():.3f} of the elements")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    assert (err <= c["bound"]).all(), f"max err/bound {worst}"
    again = call(L, c["S"], c["R"], c["mask"], c["sigma"], mode, channels, R.BLEND)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))


@pytest.mark.parametrize("channels", ["rgb", "luma"])
@pytest.mark.parametrize("name", ["overlap_3x5", "tile+1", "seg+1", "rmax_49x130"])
def test_add_of_equal_frames_keeps_the_bits(L, name, channels):
    S, _, mask, sigma = R.inputs(name)
    got = call(L, S, S.copy(), mask, sigma, "add", channels, 1.0)
    assert np.array_equal(got.view(np.int32), S.view(np.int32))


def test_wrapper_equals_the_direct_call_and_zero_blend_launches_nothing(L, monkeypatch):
    from tc_light_amd import detail
    c = R.case("tile+0", "ratio", "luma")
    s, q, m = (torch.from_numpy(c[k]).cuda() for k in ("S", "R", "mask"))
    direct = call(L, c["S"], c["R"], c["mask"], c["sigma"], "ratio", "luma", R.BLEND)
    out = detail.detail_transfer(s, q, c["sigma"], "ratio", R.BLEND, "luma", mask=m)
    torch.cuda.synchronize()
    assert out is not q and out.data_ptr() != q.data_ptr() and np.array_equal(out.cpu().numpy().view(np.int32), direct.view(np.int32))
    calls = []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(L, name)
    monkeypatch.setattr(detail, "lib", lambda: Recorder())
    assert detail.detail_transfer(s, q, c["sigma"], "ratio", 0.0, "luma", mask=m) is q and calls == []
    detail.detail_transfer(s, q, c["sigma"], "ratio", 0.5, "luma", mask=m)
    assert calls == ["tcl_detail_transfer_workspace_bytes", "tcl_detail_transfer_f32"]
    monkeypatch.undo()
    for bad, word in ((dict(source=s[:1]), "source"), (dict(source=s.double()), "source"), (dict(source=s.cpu()), "source"),
                      (dict(source=s.permute(0, 1, 3, 2)), "source"), (dict(mask=m[:, :, :-1]), "mask"), (dict(mode="mul"), "mode"),
                      (dict(channels="hsv"), "channels"), (dict(blend=1.5), "blend"), (dict(sigma=0.4), "sigma"), (dict(sigma=11.0), "radius")):
        k = dict(source=s, relit=q, sigma=c["sigma"], mode="add", blend=1.0, channels="rgb", mask=m)
        k.update(bad)
        with pytest.raises(ValueError, match=word):
            detail.detail_transfer(**k)


def test_bad_arguments_are_refused_with_nothing_written(L):
    from tc_light_amd import detail
    S, Rl, mask, sigma = R.inputs("tile+0")                      # 32 x 64, r = 6
    long_taps, _ = detail.gaussian_taps(2.5)                     # 17 taps, r = 8
    big_taps, _ = detail.gaussian_taps(16.0)                     # 97 taps, r = 48 >= min(H, W)
    bad = [dict(radius=5), dict(n_taps=11), dict(taps=long_taps, n_taps=17, radius=6), dict(taps=big_taps, n_taps=99, radius=49),
           dict(taps=big_taps, n_taps=97, radius=48), dict(H=6, W=341), dict(mode=2), dict(mode=-1), dict(luma=2), dict(blend=-0.01),
           dict(blend=1.01), dict(blend=float("nan")), dict(src=0), dict(relit=0), dict(taps=0), dict(ws=0), dict(ws_bytes=16), dict(N=0),
           dict(out="src"), dict(ws="src")]
    for change in bad:
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            call(L, S, Rl, mask, sigma, "add", "rgb", 0.5, change)
    assert L.tcl_detail_transfer_workspace_bytes(2, 32, 64, 1, 0) == 2 * 6 * 32 * 64 * 4 and L.tcl_detail_transfer_workspace_bytes(2, 32, 64, 3, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- the Generator
@pytest.fixture(scope="module")
def vae(L):
    from tc_light_amd import sd15
    from tc_light_amd.vae import VAEEngine
    return VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")


def _unet(in_channels):
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    return UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(in_channels=in_channels), seed=1), "cuda", VidToMe("cuda", seed=5))


def _generate(unet, vae, rmbg, **over):
    """The small run of tests/test_gpu_fbc.py: 2 frames of 64x64, one step, stage 1 / 2 off."""
    from tc_light_amd.generate import Generator
    from tc_light_amd.vidtome import VidToMe
    unet.tome = VidToMe("cuda", seed=5)                          # fresh draws: every run sees the same coins
    cfg = dict(n_timesteps=1, alpha_t=0.0, chunk_size=4, seed=31, noise_mode="same", apply_opt=False)
    cfg.update(over)
    g = Generator(unet, vae, cfg, rmbg=rmbg)
    gen = torch.Generator().manual_seed(9)
    frames = torch.rand(2, 3, 64, 64, generator=gen).cuda()
    conds = torch.randn(2, 77, 768, generator=gen).half().cuda()
    out, info = g(frames, conds, conds, None, None, None, source=frames if cfg.get("detail_transfer") is not None else None)
    torch.cuda.synchronize()
    return g, out, info, frames


def _check_generator(unet, vae, rmbg, **model):
    from tc_light_amd import detail
    block = dict(sigma=1.5, mode="ratio", blend=0.75, channels="luma")
    g0, plain, i0, frames = _generate(unet, vae, rmbg, **model)
    assert "detail" not in i0 and "detail" not in i0["timing"] and "detail" not in g0.timing
    g1, on, i1, _ = _generate(unet, vae, rmbg, detail_transfer=block, **model)
    mask = g1.fbc_alpha if model else None
    assert (mask is not None) == bool(model)
    want = detail.detail_transfer(frames, plain, mask=None if mask is None else mask.float().contiguous(), **block)
    torch.cuda.synchronize()
    assert torch.equal(on.view(torch.int32), want.view(torch.int32)) and not torch.equal(on, plain)
    assert i1["detail"] == block and i1["timing"]["detail"] > 0 and i1["timing"]["total"] >= i1["timing"]["detail"]
    g2, zero, i2, _ = _generate(unet, vae, rmbg, detail_transfer=dict(block, blend=0.0), **model)
    assert torch.equal(zero.view(torch.int32), plain.view(torch.int32)) and "detail" not in i2 and "detail" not in i2["timing"]
    with pytest.raises(ValueError, match="source"):              # the key without the source frames is not silently ignored
        from tc_light_amd.generate import Generator
        from tc_light_amd.vidtome import VidToMe
        unet.tome = VidToMe("cuda", seed=5)
        gg = Generator(unet, vae, dict(n_timesteps=1, apply_opt=False, detail_transfer=1.0, **model), rmbg=rmbg)
        conds = torch.zeros(2, 77, 768, dtype=torch.float16, device="cuda")
        gg(frames, conds, conds, None, None, None)


def test_generator_fc_equals_the_wrapper_on_the_plain_run(L, vae):
    _check_generator(_unet(8), vae, None)


def test_generator_fbc_takes_the_alpha_as_the_weight(L, vae):
    import warnings
    from tc_light_amd.model_utils import load_rmbg_state
    from tc_light_amd.rmbg import RMBGEngine
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rmbg = RMBGEngine(load_rmbg_state(None, allow=True), "cuda")
    _check_generator(_unet(12), vae, rmbg, iclight_model="fbc", bg_source="left")


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_with_detail(L, tmp_path):
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    import synth
    import run
    d = synth.video_clip(3, 64, 64, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    res = {}
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for name, extra in (("detail", ["--detail", "2"]), ("plain", [])):
            work = tmp_path / f"work_{name}"
            cfg = tmp_path / f"{name}.yaml"
            cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {work}
data: {{rgb_path: {vid}, height: 64, width: 64}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 1
  alpha_t: 0.01
  frame_range: [0, 3, 1]
post_opt: {{apply_opt: false}}
models: {{allow_random: true}}
""")
            run.main(["--config", str(cfg)] + extra)
            outs = [os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs if f == "output.npy"]
            assert len(outs) == 1
            out = np.load(outs[0])
            assert out.shape == (3, 64, 64, 3) and out.dtype == np.uint8
            res[name] = (out, yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))["generation"])
    finally:
        os.chdir(cwd)
    assert res["detail"][1]["detail_transfer"] == dict(sigma=2.0, mode="add", blend=1.0, channels="rgb")
    assert res["plain"][1]["detail_transfer"] is None
    diff = np.abs(res["detail"][0].astype(np.int32) - res["plain"][0].astype(np.int32))
    print(f"[run.py --detail 2] mean |difference to the plain run| = {diff.mean():.3f} of 255")
    assert diff.max() > 0
