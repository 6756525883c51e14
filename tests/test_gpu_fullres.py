"""generation.fullres on the GPU: tcl_guided_fit_f32 against the float64 reference and its derived per-element bound (tests/fullres_refs.py) on the
case table -- every window clipped, radius 1, a window larger than the image, the kernels' tile width -1 / 0 / +1 and a row segment + 1, one and three
frames, both guides, eps at its floor and at the default; tcl_guided_apply_u8 against the float64 reference's bytes on a non-integer ratio, exact 2x,
one field pixel to many and a row that ends inside a lane; the exact properties, the refusals, the wrapper and its batches, then run.py --fullres.
Outputs sit between sentinel guards."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import fullres_refs as R

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0x7FC12345                                  # a NaN bit pattern no arithmetic here produces
SENT8 = 0xA5
GEOMS = sorted(R.fit_geometries())


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, dtype=torch.float32):
    """-> (buffer of sentinels, view of `shape` inside it with GUARD sentinel elements on both sides)."""
    n = int(np.prod(shape))
    if dtype == torch.uint8:
        buf = torch.full((GUARD + n + GUARD,), SENT8, dtype=torch.uint8, device="cuda")
        return buf, buf[GUARD:GUARD + n].view(*shape)
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float32).view(*shape)


def untouched(buf):
    return bool((buf == (SENT8 if buf.dtype == torch.uint8 else SENT)).all())


def guards_kept(buf, n):
    return untouched(buf[:GUARD]) and untouched(buf[GUARD + n:])


def call_fit(L, S, Rl, r, eps, guide, change=None):
    """One direct call of the C entry on host arrays -> (abar, bbar) on the host.  change: arguments replaced to provoke a refusal, which is raised
    again after the buffers were looked at."""
    N, _, h, w = S.shape
    s, q = torch.from_numpy(S).cuda(), torch.from_numpy(Rl).cuda()
    bufa, abar = guarded(S.shape)
    bufb, bbar = guarded(S.shape)
    ws_bytes = max(L.tcl_guided_workspace_bytes(N, h, w), 4)
    bufw, ws = guarded((ws_bytes // 4,))
    k = dict(src=s, relit=q, abar=abar, bbar=bbar, N=N, h=h, w=w, radius=r, eps=R.eps32(eps), luma=R.GUIDES.index(guide), ws=ws, ws_bytes=ws_bytes)
    k.update({key: (k[v[1:]] if isinstance(v, str) and v.startswith("=") else v) for key, v in (change or {}).items()})      # "=src": alias that buffer
    refused = None
    try:
        L.tcl_guided_fit_f32(k["src"], k["relit"], k["abar"], k["bbar"], k["N"], k["h"], k["w"], k["radius"], k["eps"], k["luma"], k["ws"],
                             k["ws_bytes"], st())
    except RuntimeError as e:
        refused = e
    torch.cuda.synchronize()
    assert guards_kept(bufa, abar.numel()) and guards_kept(bufb, bbar.numel()) and guards_kept(bufw, ws.numel()), "a guard was written"
    assert torch.equal(s.cpu(), torch.from_numpy(S)) and torch.equal(q.cpu(), torch.from_numpy(Rl)), "an input was written"
    if refused is not None:                                      # a refused call writes nothing: outputs and workspace keep their fill
        assert untouched(bufa) and untouched(bufb) and untouched(bufw), f"a refused call wrote something ({change})"
        raise refused
    return abar.cpu().numpy(), bbar.cpu().numpy()


def call_apply(L, abar, bbar, src, change=None):
    N, _, h, w = abar.shape
    Hc, Wc = src.shape[1:3]
    a, b, s = torch.from_numpy(abar).cuda(), torch.from_numpy(bbar).cuda(), torch.from_numpy(src).cuda()
    buf, out = guarded(src.shape, torch.uint8)
    k = dict(abar=a, bbar=b, src=s, out=out, N=N, h=h, w=w, Hc=Hc, Wc=Wc)
    k.update({key: (k[v[1:]] if isinstance(v, str) and v.startswith("=") else v) for key, v in (change or {}).items()})
    refused = None
    try:
        L.tcl_guided_apply_u8(k["abar"], k["bbar"], k["src"], k["out"], k["N"], k["h"], k["w"], k["Hc"], k["Wc"], st())
    except RuntimeError as e:
        refused = e
    torch.cuda.synchronize()
    assert guards_kept(buf, out.numel()), "a guard next to the output was written"
    assert torch.equal(s.cpu(), torch.from_numpy(src)) and torch.equal(a.cpu(), torch.from_numpy(abar)), "an input was written"
    if refused is not None:
        assert untouched(buf), f"a refused call wrote something ({change})"
        raise refused
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("guide,eps", R.FIT_SETTINGS)
@pytest.mark.parametrize("name", GEOMS)
def test_fit_within_bound_of_float64(L, name, guide, eps, N):
    c = R.fit_case(name, guide, eps, N)
    abar, bbar = call_fit(L, c["S"], c["R"], c["r"], eps, guide)
    ea, eb = np.abs(abar.astype(np.float64) - c["abar"]), np.abs(bbar.astype(np.float64) - c["bbar"])
    worst = max((ea / c["e_abar"]).max(), (eb / c["e_bbar"]).max())
    print(f"{name} {guide} eps {eps} N {N}: max |err| abar {ea.max():.3e} bbar {eb.max():.3e}, max err/bound {worst:.3f}")
    assert np.isfinite(abar).all() and np.isfinite(bbar).all()
    assert (ea <= c["e_abar"]).all() and (eb <= c["e_bbar"]).all(), f"max err/bound {worst}"
    again = call_fit(L, c["S"], c["R"], c["r"], eps, guide)
    assert np.array_equal(abar.view(np.int32), again[0].view(np.int32)) and np.array_equal(bbar.view(np.int32), again[1].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- the apply
@pytest.mark.parametrize("name", sorted(R.APPLY_CASES))
def test_apply_equals_float64_bytes(L, name):
    abar, bbar, src = R.apply_inputs(name)
    got = call_apply(L, abar, bbar, src)
    ok, bad, near = R.apply_matches(got, abar, bbar, src)
    print(f"{name}: {bad} mismatches beyond the rule, share of values within the bound of a rounding boundary {near:.2e}, "
          f"bytes that differ from the float64 reference {(got != R.apply_reference(abar, bbar, src)[1]).mean():.2e}")
    assert ok
    assert np.array_equal(got, call_apply(L, abar, bbar, src))


@pytest.mark.parametrize("name", sorted(R.APPLY_CASES))
def test_unit_gain_returns_the_source_bytes(L, name):
    abar, bbar, src = R.apply_inputs(name)
    assert np.array_equal(call_apply(L, np.ones_like(abar), np.zeros_like(bbar), src), src)


@pytest.mark.parametrize("guide", R.GUIDES)
@pytest.mark.parametrize("s0,r0,eps", [(0.25, 0.75, R.EPS_FLOOR), (100.0 / 255.0, 180.0 / 255.0, R.EPS_DEFAULT)])
def test_constant_pair_gives_the_relit_value_everywhere(L, guide, s0, r0, eps):
    """A flat source and a flat relight: var = cov = 0 up to rounding, a ~ 0 and b ~ r0, so every native pixel becomes rn(255 r0) -- with
    s0 = 1/4, r0 = 3/4 every sum is exact and a is exactly 0, so the native bytes may be anything; the second pair applies to its own flat source."""
    N, h, w, Hc, Wc = 2, 9, 70, 21, 150
    S, Rl = np.full((N, 3, h, w), s0, np.float32), np.full((N, 3, h, w), r0, np.float32)
    abar, bbar = call_fit(L, S, Rl, 4, eps, guide)
    if s0 == 0.25:
        assert (abar == 0).all() and (bbar == np.float32(0.75)).all()
        src = np.random.default_rng(3).integers(0, 256, (N, Hc, Wc, 3), dtype=np.uint8)
    else:
        src = np.full((N, Hc, Wc, 3), 100, np.uint8)
    got = call_apply(L, abar, bbar, src)
    assert (got == int(np.rint(255.0 * r0))).all()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_bad_fit_arguments_are_refused_with_nothing_written(L):
    S, Rl = (t[:2] for t in R.fit_inputs("tile+0"))
    bad = [dict(radius=0), dict(radius=65), dict(radius=-1), dict(h=0), dict(w=0), dict(h=-3), dict(N=0), dict(N=65536), dict(h=65536, w=1),
           dict(N=1000, h=4000, w=4000), dict(eps=9e-5), dict(eps=1.5), dict(eps=0.0), dict(eps=float("nan")), dict(luma=2), dict(luma=-1),
           dict(src=0), dict(relit=0), dict(abar=0), dict(bbar=0), dict(ws=0), dict(ws_bytes=16), dict(ws_bytes=-1), dict(abar="=src"),
           dict(bbar="=abar"), dict(ws="=relit"), dict(bbar="=ws")]
    for change in bad:
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            call_fit(L, S, Rl, 3, 1e-3, "rgb", change)
    from tc_light_amd import fullres
    assert L.tcl_guided_workspace_bytes(2, 32, 64) == 2 * fullres.WS_PLANES * 32 * 64 * 4
    assert L.tcl_guided_workspace_bytes(0, 32, 64) == 0 and L.tcl_guided_workspace_bytes(1000, 4000, 4000) == 0 and L.tcl_guided_workspace_bytes(1, 65536, 1) == 0


def test_bad_apply_arguments_are_refused_with_nothing_written(L):
    abar, bbar, src = R.apply_inputs("13to37")
    bad = [dict(N=0), dict(N=65536), dict(h=0), dict(w=0), dict(Hc=0), dict(Wc=0), dict(Wc=-37), dict(Hc=65536, Wc=1), dict(N=60000, Hc=4000, Wc=4000),
           dict(N=60000, h=4000, w=4000), dict(abar=0), dict(bbar=0), dict(src=0), dict(out=0), dict(out="=src")]
    for change in bad:
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            call_apply(L, abar, bbar, src, change)


# ---------------------------------------------------------------------------------------------------------------- the wrapper
def test_wrapper_equals_the_direct_calls_and_batches_change_no_bit(L, monkeypatch):
    from tc_light_amd import fullres
    c = R.fit_case("tile+1", "luma", R.EPS_DEFAULT, 3)
    N, _, h, w = c["S"].shape
    native = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (N, 2 * h + 3, 2 * w + 5, 3), dtype=np.uint8))
    crop = (1, 2, 2 * h, 2 * w + 1)
    abar, bbar = call_fit(L, c["S"], c["R"], c["r"], R.EPS_DEFAULT, "luma")
    nat = native[:, 1:1 + 2 * h, 2:2 + 2 * w + 1].contiguous().numpy()
    direct = call_apply(L, abar, bbar, nat)
    s, q = torch.from_numpy(c["S"]).cuda(), torch.from_numpy(c["R"]).cuda()
    fa, fb = fullres.guided_fit(s, q, c["r"], R.EPS_DEFAULT, "luma")
    assert np.array_equal(fa.cpu().numpy().view(np.int32), abar.view(np.int32)) and np.array_equal(fb.cpu().numpy().view(np.int32), bbar.view(np.int32))
    assert np.array_equal(fullres.guided_apply(fa, fb, torch.from_numpy(nat).cuda()).cpu().numpy(), direct)
    calls = []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(L, name)
    monkeypatch.setattr(fullres, "lib", lambda: Recorder())
    whole = fullres.fullres(s, q, native, c["r"], R.EPS_DEFAULT, "luma", crop=crop)
    assert calls == ["tcl_guided_workspace_bytes", "tcl_guided_fit_f32", "tcl_guided_apply_u8"]
    assert whole.dtype == torch.uint8 and not whole.is_cuda and np.array_equal(whole.numpy(), direct)
    del calls[:]
    cap = fullres.bytes_per_frame(h, w, crop[2], crop[3])          # room for exactly one frame
    assert fullres.batch_size(h, w, crop[2], crop[3], cap) == 1
    one_by_one = fullres.fullres(s, q, native, c["r"], R.EPS_DEFAULT, "luma", crop=crop, cap_bytes=cap)
    assert calls == ["tcl_guided_workspace_bytes", "tcl_guided_fit_f32", "tcl_guided_apply_u8"] * N
    assert np.array_equal(one_by_one.numpy(), direct)
    monkeypatch.undo()
    for bad, word in ((dict(source=s[:1]), "source"), (dict(source=s.double()), "source"), (dict(source=s.cpu()), "source"),
                      (dict(native=native.cuda()), "native"), (dict(native=native[:2]), "native"), (dict(native=native.float()), "native"),
                      (dict(radius=0), "radius"), (dict(eps=2.0), "eps"), (dict(guide="hsv"), "guide"), (dict(crop=(0, 0, 2 * h + 4, 4)), "crop")):
        k = dict(source=s, relit=q, native=native, radius=2, eps=1e-3, guide="rgb", crop=crop)
        k.update(bad)
        with pytest.raises(ValueError, match=word):
            fullres.fullres(**k)


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_with_fullres(L, tmp_path):
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    import synth
    import run
    from tc_light_amd import fullres
    from tc_light_amd.dataparser import VideoDataParser
    d = synth.video_clip(3, 128, 128, seed=2)                    # the native clip: twice the working size
    vid = tmp_path / "clip.npy"
    u8 = (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)
    np.save(vid, u8)
    res = {}
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for name, extra in (("fullres", ["--fullres", "2"]), ("plain", [])):
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
            files = sorted(f for f in os.listdir(os.path.dirname(outs[0])) if f.startswith("output_fullres"))
            res[name] = (np.load(outs[0]), yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))["generation"], files,
                         os.path.dirname(outs[0]))
    finally:
        os.chdir(cwd)
    out, gen, files, path = res["fullres"]
    geo = R.geometry(128, 128, 64, 64)
    assert (geo["Y0"], geo["X0"], geo["Hc"], geo["Wc"]) == (0, 0, 128, 128)
    assert gen["fullres"] == dict(radius=2, eps=1e-3, guide="rgb") and gen["fullres_size"] == [128, 128]
    assert "output_fullres.npy" in files and len(files) >= 2      # the array and the video (or its stand-in)
    full = np.load(os.path.join(path, "output_fullres.npy"))
    assert full.shape == (3, 128, 128, 3) and full.dtype == np.uint8
    # the wrapper on that run's own output and source
    parser = VideoDataParser(dict(rgb_path=str(vid), height=64, width=64), "cuda")
    source = parser.load_video([0, 1, 2])
    native = parser.native_u8([0, 1, 2])
    assert np.array_equal(native.numpy(), u8)
    relit = torch.from_numpy(out).cuda().permute(0, 3, 1, 2).float() / 255.0
    want = fullres.fullres(source.float().contiguous(), relit.contiguous(), native, 2, 1e-3, "rgb", crop=(0, 0, 128, 128))
    assert np.array_equal(full, want.numpy())
    half = full.reshape(3, 64, 2, 64, 2, 3).astype(np.float64).mean(axis=(2, 4))
    print(f"[run.py --fullres 2] mean |2x2 mean of output_fullres - output| = {np.abs(half - out).mean():.3f} of 255")
    # the same run without the key
    assert np.array_equal(res["plain"][0], out) and res["plain"][2] == [] and res["plain"][1]["fullres"] is None
    assert "fullres_size" not in res["plain"][1]
