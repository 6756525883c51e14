"""generation.keyframes on the GPU: tcl_flow_chain_f32 and tcl_keyframe_propagate_f32 on exact planted motion and on a static clip, against the float64
reference and its derived per-element bound on every case of the table (tests/keyframe_refs.py), the wrapper against the direct calls, the refusals, then
the step inside the Generator and run.py --keyframes.  Outputs sit between sentinel guards.

Measured on an MI355X (max |err| / bound over the compared pixels, share of pixels left out): see the printed line of each case; the f32 emulation of
tests/test_keyframe_refs_cpu.py sits at 0.09 - 0.24 of the bound."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import keyframe_refs as R

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0x7FC12345                                  # a NaN bit pattern no arithmetic here produces
NAMES = sorted(R.CASES)


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


def direct(L, S, Rk, fut, past, keys, alpha=R.ALPHA, thr=R.DIFF, eps=R.EPS, change=None, only=None):
    """The two C entries, batch by batch, on host arrays -> (out, holes, chains [span,2,3,H,W] of the LAST batch) on the host.  change: arguments
    replaced to provoke a refusal (`only`: of that entry alone), raised again after the buffers were looked at."""
    from tc_light_amd import keyframe
    N, _, H, W = S.shape
    h_keys, h_left, h_right, h_tw = keyframe.tables(keys, N)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S, Rk, fut, past)]
    obuf, out = guarded(S.shape)
    hbuf, holes = guarded((N,), torch.int32)
    ws_bytes = max(L.tcl_keyframe_workspace_bytes(N, H, W, max([b - a for a, b in zip(keys, keys[1:])] or [1])), 4)
    wbuf, ws = guarded((ws_bytes // 4,))
    k = dict(source=dev[0], relit=dev[1], fut=dev[2], past=dev[3], out=out, holes=holes, h_keys=h_keys, M=len(keys), h_left=h_left, h_right=h_right,
             h_tw=h_tw, N=N, H=H, W=W, alpha=alpha, thr=thr, eps=eps, ws=ws, ws_bytes=ws_bytes)
    refused = None
    span = 0
    try:
        for g0, g1 in keyframe.batches(keys) or [(0, 0)]:
            a = dict(k, g0=g0, g1=g1)
            c = dict(a, **(change or {}))
            a1, a2 = (c if only in (None, "chain") else a), (c if only in (None, "propagate") else a)
            if only != "propagate" or change is None:
                L.tcl_flow_chain_f32(a1["fut"], a1["past"], a1["h_keys"], a1["M"], a1["g0"], a1["g1"], a1["N"], a1["H"], a1["W"], a1["alpha"],
                                     a1["ws"], a1["ws_bytes"], st())
            if only != "chain" or change is None:
                L.tcl_keyframe_propagate_f32(a2["source"], a2["relit"], a2["out"], a2["holes"], a2["h_keys"], a2["M"], a2["g0"], a2["g1"],
                                             a2["h_left"], a2["h_right"], a2["h_tw"], a2["N"], a2["H"], a2["W"], a2["thr"], a2["eps"], a2["ws"],
                                             a2["ws_bytes"], st())
            span = keys[g1] - keys[g0] + 1
    except RuntimeError as e:
        refused = e
    torch.cuda.synchronize()
    assert guards_kept(obuf, out.numel()) and guards_kept(hbuf, N) and guards_kept(wbuf, ws.numel()), "a guard next to an output was written"
    for t, a in zip(dev, (S, Rk, fut, past)):
        assert torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a))), "an input was written"
    if refused is not None:
        assert bool((obuf == SENT).all()) and bool((hbuf == SENT).all()) and bool((wbuf == SENT).all()), f"a refused call wrote something ({change})"
        raise refused
    chains = ws[:span * 6 * H * W].view(span, 2, 3, H, W).cpu().numpy() if span else None
    return out.cpu().numpy(), holes.cpu().numpy(), chains


def test_tile_constants_are_the_headers():
    from tc_light_amd import keyframe
    assert (keyframe.TILE_W, keyframe.TILE_H) == (R.TILE_W, R.TILE_H)


def test_exact_planted_motion(L):
    """A texture translated by an integer vector per frame, relit keys = source * a gain that moves with the texture: inside both keys the frames in
    between are source * gain to planted_bound; the strip entering the frame (content in neither key) is exactly the holes; keys bit for bit.
    "In a key" is what the header states: d steps of u pixels towards the key stay inside the frame, and, from the second step on, so do the four
    taps (x0 | x0 + 1, y0 | y0 + 1) of the chain of the step before -- where u > 0 the far tap costs one more pixel per step: x + d u + (d - 1) <= W - 1;
    where u < 0: x + d u >= 0; u = 0: always."""
    N, K, H, W = 9, 4, 37, 70
    keys = R.keyframe_ids(N, K)
    rng = np.random.default_rng(5)
    pad = 40
    canvas = np.round(R._texture(rng, H + 2 * pad, W + 2 * pad) * 256) / 256            # multiples of 2^-8: s + eps is exact
    gain = (0.5 + R._texture(rng, H + 2 * pad, W + 2 * pad, waves=3, lo=0.0, hi=1.0)[:1]).astype(np.float32)
    v = np.array([[3, 1]] * 4 + [[-2, 1]] * 4)                                          # (dx, dy) of frame i -> i+1: content moves by v
    o = np.concatenate([[[0, 0]], -np.cumsum(v, axis=0)]) + pad                         # frame i shows the canvas from offset o_i
    S = np.stack([canvas[:, o[i, 1]:o[i, 1] + H, o[i, 0]:o[i, 0] + W] for i in range(N)]).astype(np.float32)
    Gn = np.stack([gain[:, o[i, 1]:o[i, 1] + H, o[i, 0]:o[i, 0] + W] for i in range(N)])
    fut = np.zeros((N, 2, H, W), dtype=np.float32); past = np.zeros_like(fut)
    for i in range(N - 1):
        fut[i] = v[i][:, None, None]
        past[i + 1] = -v[i][:, None, None]
    relit_all = (S * Gn).astype(np.float32)                                             # one f32 multiplication
    out, holes, _ = direct(L, S, relit_all[keys], fut, past, keys)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for i in range(N):
        if i in keys:
            assert np.array_equal(out[i].view(np.int32), relit_all[i].view(np.int32)) and holes[i] == 0
            continue
        a = max(k for k in keys if k < i); b = min(k for k in keys if k > i)
        inside = []
        for key in (a, b):                                                              # is the content of p in frame i in the key?
            d, u = abs(key - i), (v[a] if key == b else -v[a])                          # the gap's motion is constant: u per step towards the key
            ok = np.ones((H, W), dtype=bool)
            for coord, step, size in ((xs, u[0], W), (ys, u[1], H)):
                if step > 0:
                    ok &= coord + d * step + (d - 1) <= size - 1
                elif step < 0:
                    ok &= coord + d * step >= 0
            inside.append(ok)
        both, none = inside[0] & inside[1], ~inside[0] & ~inside[1]
        want = S[i].astype(np.float64) * Gn[i].astype(np.float64)
        err = np.abs(out[i].astype(np.float64) - want)
        bound = R.planted_bound(want) + R.U * np.abs(want)                              # relit_all's own rounding is part of planted_bound; want is exact
        seen = inside[0] | inside[1]
        print(f"frame {i}: max err/bound inside a key {(err / bound)[:, seen].max():.3f}, holes {holes[i]} (strip {int(none.sum())})")
        assert (err <= bound)[:, both].all() and (err <= bound)[:, seen].all()
        assert holes[i] == int(none.sum())


def test_static_clip(L):
    """Zero flows and equal source frames: the output is ta R_a + tb R_b."""
    N, K, H, W = 6, 4, 33, 129
    keys = R.keyframe_ids(N, K)
    rng = np.random.default_rng(6)
    S0 = (np.round(R._texture(rng, H, W) * 256) / 256).astype(np.float32)
    S = np.stack([S0] * N)
    Rk = np.stack([(S0 * (0.6 + 0.2 * k)).astype(np.float32) for k in range(len(keys))])
    z = np.zeros((N, 2, H, W), dtype=np.float32)
    out, holes, chains = direct(L, S, Rk, z, z, keys)
    _, _, tw = R.tables(keys, N)
    assert holes.sum() == 0
    for i in range(N):
        if i in keys:
            continue
        ka = max(k for k in range(len(keys)) if keys[k] < i)
        want = float(tw[0, i]) * Rk[ka].astype(np.float64) + float(tw[1, i]) * Rk[ka + 1].astype(np.float64)
        err = np.abs(out[i].astype(np.float64) - want)
        assert (err <= R.planted_bound(want)).all(), (i, (err / R.planted_bound(want)).max())


@pytest.mark.parametrize("name", NAMES)
def test_kernel_within_bound_of_float64(L, name):
    c = R.case(name)
    keys = c["keys"]
    out, holes, chains = direct(L, c["S"], c["R"], c["fut"], c["past"], keys)
    keep = ~c["left_out"][:, None].repeat(3, axis=1)
    err = np.abs(out.astype(np.float64) - c["out"]) / np.maximum(c["bound"], 1e-300)
    share = float(c["left_out"].mean())
    assert np.isfinite(out).all()
    worst = float(err[keep].max())
    print(f"{name}: max err/bound {worst:.3f}, left out {share:.4f}, holes {holes.tolist()} (reference {c['holes'].tolist()})")
    assert share <= R.MAX_AMBIGUOUS
    assert worst <= 1.0
    for k, key in enumerate(keys):
        assert np.array_equal(out[key].view(np.int32), c["R"][k].view(np.int32))
    # holes: exact where no pixel of the frame is ambiguous, else within the ambiguous pixels
    slack = c["left_out"].reshape(len(out), -1).sum(axis=1)
    assert (np.abs(holes.astype(np.int64) - c["holes"]) <= slack).all()
    if R.CASES[name][4] == "integer":
        assert np.array_equal(holes, c["holes"])
    if chains is not None and len(keys) > 1:                        # the chains of the last batch (these clips have one): valid and flow as stated
        from tc_light_amd import keyframe
        f0 = keys[keyframe.batches(keys)[-1][0]]
        for s in range(chains.shape[0]):
            j = f0 + s
            if j in keys:
                continue
            ok = ~c["amb"][j]
            assert np.array_equal(chains[s, :, 2][ok], c["C"][j, :, 2][ok])
            d = np.abs(chains[s, :, :2].astype(np.float64) - c["C"][j, :, :2])
            assert (d <= R.SAFETY * c["E"][j][:, None] + 1e-12)[np.broadcast_to(ok[:, None], d.shape)].all()
    again, holes2, _ = direct(L, c["S"], c["R"], c["fut"], c["past"], keys)
    assert np.array_equal(out.view(np.int32), again.view(np.int32)) and np.array_equal(holes, holes2)


def test_wrapper_equals_the_direct_calls_and_interval_one_launches_nothing(L, monkeypatch):
    from tc_light_amd import keyframe
    c = R.case("n9k4_37x70_smooth")
    s, r, fu, pa = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("S", "R", "fut", "past"))
    want, wholes, _ = direct(L, c["S"], c["R"], c["fut"], c["past"], c["keys"])
    out, holes = keyframe.propagate(s, r, c["keys"], fu, pa, R.ALPHA, R.DIFF, R.EPS)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)) and np.array_equal(holes.cpu().numpy(), wholes)
    # a clip longer than one batch: a smooth texture translated by an integer vector per frame, so both gates are open and the warped path runs on
    # both sides of the key frame the two batches share; both give what the reference gives
    N, H, W = 41, 9, 70
    rng = np.random.default_rng(3)
    keys = R.keyframe_ids(N, 4)
    pad = 48
    canvas = R._texture(rng, H + 2 * pad, W + 2 * pad)
    v = np.round(rng.uniform(-1, 1, size=(N, 2))).astype(np.int64)               # (dx, dy) of frame i -> i+1
    o = np.concatenate([[[0, 0]], -np.cumsum(v[:-1], axis=0)]) + pad             # frame i shows the canvas from offset o_i (|o - pad| <= 40)
    S = np.stack([canvas[:, o[i, 1]:o[i, 1] + H, o[i, 0]:o[i, 0] + W] for i in range(N)]).astype(np.float32)
    Rk = (S[keys] * rng.uniform(0.6, 1.4, size=(len(keys), 3, H, W))).astype(np.float32)
    fut = np.zeros((N, 2, H, W), dtype=np.float32); past = np.zeros_like(fut)
    for i in range(N - 1):
        fut[i] = v[i][:, None, None]
        past[i + 1] = -v[i][:, None, None]
    assert len(keyframe.batches(keys)) > 1
    o2, h2 = keyframe.propagate(*(torch.from_numpy(a).cuda() for a in (S, Rk)), keys, torch.from_numpy(fut).cuda(), torch.from_numpy(past).cuda())
    C, E, amb = R.chain_ref(fut, past, keys)
    ref, rholes, bound, left_out = R.propagate_ref(S, Rk, keys, C, E, amb)
    keep = ~left_out[:, None].repeat(3, axis=1)
    err = np.abs(o2.cpu().numpy().astype(np.float64) - ref) / np.maximum(bound, 1e-300)
    assert err[keep].max() <= 1.0 and left_out.mean() <= R.MAX_AMBIGUOUS
    seam = keys[keyframe.batches(keys)[0][1]]                                   # the shared key frame: warped pixels on both sides of it
    assert all(rholes[i] < 0.5 * H * W for i in (seam - 1, seam + 1)) and (C[[seam - 1, seam + 1], :, 2].mean(axis=(2, 3)) > 0.5).all()
    assert (np.abs(h2.cpu().numpy() - rholes) <= left_out.reshape(N, -1).sum(axis=1)).all()
    calls = []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(L, name)
    monkeypatch.setattr(keyframe, "lib", lambda: Recorder())
    every = list(range(len(c["S"])))
    same, zero = keyframe.propagate(s, s.clone(), every, fu, pa)
    assert calls == [] and int(zero.sum()) == 0
    rk = s.clone()
    assert keyframe.propagate(s, rk, every, fu, pa)[0] is rk and calls == []
    keyframe.propagate(s, r, c["keys"], fu, pa)
    assert calls == ["tcl_keyframe_workspace_bytes", "tcl_flow_chain_f32", "tcl_keyframe_propagate_f32"]
    monkeypatch.undo()
    for bad, word in ((dict(source=s[:5]), "keys"), (dict(source=s.double()), "source"), (dict(source=s.cpu()), "source"),
                      (dict(source=s.permute(0, 1, 3, 2)), "source"), (dict(relit_keys=r[:2]), "relit_keys"), (dict(fut=fu[:, :1]), "fut"),
                      (dict(past=pa.half()), "past"), (dict(keys=[0, 4, 7]), "keys"), (dict(alpha=0.0), "alpha"), (dict(diff_threshold=-1.0), "diff"),
                      (dict(eps=0.5), "eps")):
        k = dict(source=s, relit_keys=r, keys=c["keys"], fut=fu, past=pa, alpha=0.1, diff_threshold=0.1, eps=R.EPS)
        k.update(bad)
        with pytest.raises(ValueError, match=word):
            keyframe.propagate(**k)


def test_bad_arguments_are_refused_with_nothing_written(L):
    c = R.case("n6k4_33x129_integer")                            # keys 0, 4, 5
    N = 6
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    both = [dict(h_keys=0), dict(ws=0), dict(N=0), dict(H=0), dict(W=-1), dict(M=0), dict(h_keys=i32([0, 4, 4])), dict(h_keys=i32([1, 4, 5])),
            dict(h_keys=i32([0, 3, 4])), dict(h_keys=i32([0, 5, 4])), dict(g0=-1), dict(g1=3), dict(g0=2, g1=1), dict(ws_bytes=16)]
    chain = [dict(fut=0), dict(past=0), dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf"))]
    prop = [dict(source=0), dict(relit=0), dict(out=0), dict(holes=0), dict(h_left=0), dict(h_right=0), dict(h_tw=0), dict(thr=0.0),
            dict(thr=float("nan")), dict(eps=0.0), dict(eps=0.26), dict(eps=float("nan")), dict(h_left=i32([0, 0, 0, 0, 1, 1])),
            dict(h_right=i32([0, 1, 1, 1, 2, 2])), dict(h_tw=torch.full((2, N), 1.5))]
    for only, changes in (("chain", both + chain), ("propagate", both + prop)):
        for change in changes:
            with pytest.raises(RuntimeError, match="TCL_EINVAL"):
                direct(L, c["S"], c["R"], c["fut"], c["past"], c["keys"], change=change, only=only)
    # a gap above TCL_KEYFRAME_MAX_GAP
    from tc_light_amd import keyframe
    far = i32([0, 17])
    z = torch.zeros(18, 2, 4, 64, device="cuda")
    ws = torch.zeros(33 * 6 * 4 * 64, device="cuda")
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_flow_chain_f32(z, z, far, 2, 0, 1, 18, 4, 64, 0.1, ws, ws.numel() * 4, st())
    assert L.tcl_keyframe_workspace_bytes(100, 8, 16, 4) == keyframe.BATCH_FRAMES * 24 * 8 * 16
    assert L.tcl_keyframe_workspace_bytes(5, 8, 16, 4) == 5 * 24 * 8 * 16
    assert L.tcl_keyframe_workspace_bytes(5, 8, 16, 17) == 0 and L.tcl_keyframe_workspace_bytes(5, 8, 16, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- the Generator
@pytest.fixture(scope="module")
def engines(L):
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vae import VAEEngine
    from tc_light_amd.vidtome import VidToMe
    vae = VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")
    unet = UNetEngine(sd15.random_state_dict(sd15.unet_param_shapes(in_channels=8), seed=1), "cuda", VidToMe("cuda", seed=5))
    return unet, vae


def _clip():
    gen = torch.Generator().manual_seed(9)
    frames = torch.rand(5, 3, 64, 64, generator=gen).cuda()
    conds = torch.randn(2, 77, 768, generator=gen).half().cuda()
    fut = (torch.rand(5, 2, 64, 64, generator=gen) * 2 - 1).cuda()
    past = (torch.rand(5, 2, 64, 64, generator=gen) * 2 - 1).cuda()
    fut[-1] = 0; past[0] = 0
    return frames, conds, fut, past


def _generate(engines, frames, conds, call=None, **over):
    """The small run of tests/test_gpu_detail.py: 64x64, one step, stage 1 / 2 off."""
    from tc_light_amd.generate import Generator
    from tc_light_amd.vidtome import VidToMe
    unet, vae = engines
    unet.tome = VidToMe("cuda", seed=5)                          # fresh draws: every run sees the same coins
    cfg = dict(n_timesteps=1, alpha_t=0.0, chunk_size=4, seed=31, noise_mode="same", apply_opt=False)
    cfg.update(over)
    g = Generator(unet, vae, cfg)
    out, info = g(frames, conds, conds, None, None, None, **(call or {}))
    torch.cuda.synchronize()
    return out, info


def test_generator_denoises_the_keys_and_propagates_the_rest(L, engines):
    from tc_light_amd import keyframe
    frames, conds, fut, past = _clip()
    keys = [0, 2, 4]
    plain3, i3 = _generate(engines, frames[keys].contiguous(), conds)
    assert "keyframes" not in i3 and "propagate" not in i3["timing"]
    call = dict(source=frames, flows=(fut, past), keyframes=keys, n_total=3)
    on, info = _generate(engines, frames[keys].contiguous(), conds, call, keyframes=2)
    assert on.shape == (5, 3, 64, 64)
    assert torch.equal(on[keys].view(torch.int32), plain3.view(torch.int32))
    want, holes = keyframe.propagate(frames, plain3.float().contiguous(), keys, fut, past)
    torch.cuda.synchronize()
    assert torch.equal(on.view(torch.int32), want.view(torch.int32))
    assert info["keyframes"]["denoised"] == 3 and info["keyframes"]["interval"] == 2
    assert info["keyframes"]["holes"] == int(holes.sum()) / (2 * 64 * 64)
    assert info["timing"]["propagate"] > 0 and info["total_number_of_frames"] == 5
    assert abs(info["sec_per_frame"] - info["total_time"] / 5) < 1e-12
    # interval 1: the plain 5-frame run bit for bit, nothing recorded
    plain5, _ = _generate(engines, frames, conds)
    one, i1 = _generate(engines, frames, conds, dict(source=frames, flows=(fut, past), keyframes=list(range(5))), keyframes=1)
    assert torch.equal(one.view(torch.int32), plain5.view(torch.int32)) and "keyframes" not in i1 and "propagate" not in i1["timing"]
    one, i1 = _generate(engines, frames, conds, keyframes=1)
    assert torch.equal(one.view(torch.int32), plain5.view(torch.int32)) and "keyframes" not in i1
    for missing in ("source", "flows", "keyframes"):
        with pytest.raises(ValueError, match=missing):
            _generate(engines, frames[keys].contiguous(), conds, {k: v for k, v in call.items() if k != missing}, keyframes=2)


# ---------------------------------------------------------------------------------------------------------------- run.py
def _run_config(tmp_path, root, vid, name, apply_opt, extra=""):
    work = tmp_path / f"work_{name}"
    cfg = tmp_path / f"{name}.yaml"
    cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {work}
data: {{rgb_path: {vid}, height: 192, width: 256, flow_model: raft{extra}}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 1
  alpha_t: 0.01
  frame_range: [0, 5, 1]
post_opt: {{apply_opt: {'true' if apply_opt else 'false'}, epochs_exposure: 1, epochs: 1, batch_size: 4}}
models: {{allow_random: true, raft: {tmp_path / 'absent' / 'raft-things.pth'}}}
""")
    return work, cfg


def test_run_py_with_keyframes(L, tmp_path):
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    import synth
    import run
    # 192x256, the clip size of test_gpu_raft_run.py: RAFT takes no side below 128 (raft.check_size) and stage 1's MS-SSIM none below 176
    d = synth.video_clip(5, 192, 256, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for name, apply_opt in (("noopt", False), ("opt", True)):
            work, cfg = _run_config(tmp_path, root, vid, name, apply_opt)
            run.main(["--config", str(cfg), "--keyframes", "2"])
            outs = [os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs if f == "output.npy"]
            assert len(outs) == 1
            out = np.load(outs[0])
            assert out.shape == (5, 192, 256, 3) and out.dtype == np.uint8
            rec = yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))
            assert rec["generation"]["keyframes"] == dict(interval=2, alpha=0.1, diff_threshold=0.1, eps=0.015625)
            assert rec["generation"]["keyframes_denoised"] == 3 and 0.0 <= rec["generation"]["keyframes_holes"] <= 1.0
            assert rec["total_number_of_frames"] == 5
        # out of scope beside the key: refused before any model is loaded
        loaded = []
        real = run.init_iclight
        run.init_iclight = lambda *a, **k: loaded.append(1) or real(*a, **k)
        try:
            for name, lines, words in (("normal", ["--normal", "--iclight_model", "fbc"], ("generation.keyframes", "generation.normal")),
                                       ("light", ["--light_sweep", "0", "90", "--strength", "1"], ("generation.keyframes", "generation.light_path")),
                                       ("prompt", ["--prompt_sweep", "dawn", "dusk"], ("generation.keyframes", "generation.prompt_path"))):
                work, cfg = _run_config(tmp_path, root, vid, name, False)
                with pytest.raises(ValueError) as e:
                    run.main(["--config", str(cfg), "--keyframes", "2"] + lines)
                assert all(w in str(e.value) for w in words), str(e.value)
            work, cfg = _run_config(tmp_path, root, vid, "sceneflow", False, extra=", scene_type: sceneflow")
            with pytest.raises(ValueError) as e:
                run.main(["--config", str(cfg), "--keyframes", "2"])
            assert "generation.keyframes" in str(e.value) and "data.scene_type" in str(e.value)
        finally:
            run.init_iclight = real
        assert loaded == []
    finally:
        os.chdir(cwd)
