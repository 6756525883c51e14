"""GPU: frame-lpips (csrc/lpips.hip, tc_light_amd/lpips.py, tc_light_amd/evaluate.py frame_lpips, evaluate.py --lpips) against the float64 restatement
tests/lpips_refs.py and tests/golden/lpips.npz.  Leaves first (stem, pool, head + finish) at the smallest shapes at which each can go wrong, then
the engine against the exact and the f16-floor references, the whole figure, the command line and the refusals.  The figures of an MI355X run are in
profiles/lpips_parity.txt (this file's output under `pytest -s`)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
U16, U32 = 2.0 ** -11, 2.0 ** -24                 # unit round-offs of f16 and f32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def state():
    return R.seeded_state(8)


@pytest.fixture(scope="module")
def engine(dev, state):
    from tc_light_amd.lpips import LPIPSEngine
    return LPIPSEngine(state, dev)


def _L():
    from tc_light_amd.lib import lib, stream
    return lib(), stream()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- stem
def _stem(dev, img, w27, bias, shift):
    L, st = _L()
    B, H, W = img.shape[:3]
    y = torch.empty(B, H, W, 64, dtype=torch.float16, device=dev)
    L.tcl_lpips_stem_f16(img.to(dev), w27.to(dev), bias.to(dev), float(shift[0]), float(shift[1]), float(shift[2]), y, B, H, W, st)
    return y.cpu()


def _stem_f64(img, w27, bias, shift, pad_before=False):
    """-> (pre-ReLU sums, the sum of the absolute terms), float64 [B,H,W,64], from the f32 operands the kernel gets.  pad_before: the WRONG rule
    (the uint8 image padded with 0, then shifted), for the border check."""
    x = img.permute(0, 3, 1, 2).to(F64)
    sh = torch.tensor([float(np.float32(s)) for s in shift], dtype=F64).view(1, 3, 1, 1)
    w = w27.to(F64).view(64, 3, 3, 3).permute(0, 3, 1, 2)                              # [o, (ky, kx, c)] -> [o, c, ky, kx]
    v = (F.pad(x, [1, 1, 1, 1]) - sh) if pad_before else F.pad(x - sh, [1, 1, 1, 1])
    s = F.conv2d(v, w, bias.to(F64))
    a = F.conv2d(v.abs(), w.abs(), bias.to(F64).abs())
    return s.permute(0, 2, 3, 1), a.permute(0, 2, 3, 1)


def _ulp16(x):
    """The spacing of f16 at |x| (float64 tensor); subnormal spacing 2^-24 below 2^-14."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def _border_image(seed, B, H, W):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    img[:, 0], img[:, -1], img[:, :, 0], img[:, :, -1] = 255, 180, 230, 140            # far from the shift colour (about 0)
    return torch.from_numpy(img)


def test_stem_vs_f64_every_pixel(dev, state):
    """B = 2, 9 x 13 (13 pixels of a row straddle the 32-pixel groups of a block).  Bound per element: half an f16 ulp of the float64 value (the one
    rounding) plus the f32 arithmetic before it, 29 u32 times the sum of the absolute terms (one rounding for x - shift, one per product, at most 27
    per running sum), which matters only where the terms cancel."""
    from tc_light_amd.lpips import INPUT_SCALE, SCALE, SHIFT
    img = _border_image(1, 2, 9, 13)
    fold = (INPUT_SCALE / torch.tensor(SCALE, dtype=F64)).view(1, 3, 1, 1)
    w27 = (state["features.0.weight"].double() * fold).permute(0, 2, 3, 1).reshape(64, 27).float().contiguous()
    bias = (state["features.0.bias"].double() * INPUT_SCALE).float()
    got = _stem(dev, img, w27, bias, SHIFT).to(F64)
    s, a = _stem_f64(img, w27, bias, SHIFT)
    ref = s.clamp_min(0)
    tol = 0.5 * _ulp16(ref) + 29 * U32 * a
    err = (got - ref).abs()
    print(f"stem 2x9x13: max |err| / tol {float((err / tol).max()):.3f}; max |err| {float(err.max()):.3e}")
    assert (err <= tol).all(), f"worst pixel {np.unravel_index(int((err / tol).argmax()), err.shape)}: {float(err.max())}"
    for yy, xx in ((0, 0), (0, 12), (8, 0), (8, 12)):                                  # the four corners, by name
        assert (err[:, yy, xx] <= tol[:, yy, xx]).all()


def test_stem_lattice_weights_bit_for_bit(dev):
    """Weights k / 16 with |k| <= 8, biases k / 16, shifts in quarters: x - shift has 11 significant bits, a product 15, and the 28-term sum stays below
    2^12 with a granularity of 2^-6: every operation is exact in f32, so the kernel must return the f16 rounding of the exact value, bit for bit."""
    g = np.random.default_rng(2)
    img = _border_image(3, 2, 9, 13)
    w27 = torch.from_numpy(g.integers(-8, 9, (64, 27)).astype(np.float32) / 16)
    bias = torch.from_numpy(g.integers(-64, 65, 64).astype(np.float32) / 16)
    shift = (-0.5, 1.25, -2.0)
    got = _stem(dev, img, w27, bias, shift)
    s, a = _stem_f64(img, w27, bias, shift)
    assert float(a.max()) < 2.0 ** 12 and torch.equal(s * 64, (s * 64).round())
    want = s.clamp_min(0).to(torch.float16)
    assert float(want.float().max()) > 100 and (want == 0).any()
    assert torch.equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} of {want.numel()} elements differ"
    # the wrong border rule (the uint8 image padded with 0, then shifted) gives other bits on every border pixel and only there: the test looks there
    wrong = _stem_f64(img, w27, bias, shift, pad_before=True)[0].clamp_min(0).to(torch.float16)
    differs = (_bits(wrong) != _bits(want)).any(-1)
    border = torch.ones(9, 13, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert differs[:, border].all() and not differs[:, ~border].any()


# ---------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("H,W,C", [(7, 10, 64), (8, 9, 128)])
def test_maxpool_bit_equal_to_torch(dev, H, W, C):
    L, st = _L()
    g = np.random.default_rng(H * W)
    x = torch.from_numpy(g.integers(-3, 4, (2, H, W, C)).astype(np.float32) / 2).half()          # few distinct values: ties in most windows
    z = torch.from_numpy(g.random((2, H, W, C)))
    x[z < 0.25] = 0.0
    x[z < 0.12] = -0.0
    x[(z > 0.97)] = 65504.0
    x[(z > 0.985)] = -65504.0
    y = torch.empty(2, H // 2, W // 2, C, dtype=torch.float16, device=dev)
    L.tcl_maxpool2_f16(x.to(dev), y, 2, H, W, C, st)
    want = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 2, 2).permute(0, 2, 3, 1)
    neg0 = int((_bits(want) == -32768).sum())
    assert neg0 > 0 and int((want == 0).sum()) > neg0 and (want == 65504).any()                   # both zeros and the largest finite f16 among the results
    assert torch.equal(_bits(y.cpu()), _bits(want))


# ---------------------------------------------------------------------------------------------------------------- head + finish
def _head(dev, feats, ws_list, B, eps):
    """feats: one [2B,P,C] f16 tensor per tap, ws_list: one [C] f32 per tap -> (out [B] f32, nonfinite [ntaps]) on the host."""
    L, st = _L()
    P = [f.shape[1] for f in feats]
    h_P = torch.tensor(P, dtype=torch.int32)
    ws = torch.empty(sum(B * (-(-p // 64)) * 8 for p in P), dtype=torch.uint8, device=dev)
    for k, (f, w) in enumerate(zip(feats, ws_list)):
        L.tcl_lpips_head(f.to(dev).contiguous(), w.to(dev), B, h_P, len(P), k, f.shape[2], eps, ws, st)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    bad = torch.full((len(P),), -1, dtype=torch.int32, device=dev)
    L.tcl_lpips_finish(ws, B, h_P, len(P), out, bad, st)
    return out.cpu(), bad.cpu()


def _head_f64(f, w, B, eps):
    """-> (d [B], A [B]) float64 on the f16 features: the distance and A = mean over the pixels of sum_c w_c 2 |n0 - n1| (|n0| + |n1|)."""
    f = f.to(F64)
    f0, f1 = f[:B], f[B:]
    n0 = f0 / (f0.pow(2).sum(-1, keepdim=True).sqrt() + eps)
    n1 = f1 / (f1.pow(2).sum(-1, keepdim=True).sqrt() + eps)
    w = w.to(F64)
    return ((n0 - n1).pow(2) * w).sum(-1).mean(-1), (2 * (n0 - n1).abs() * (n0.abs() + n1.abs()) * w).sum(-1).mean(-1)


def _head_tol(d, A, C):
    """The f32 bound.  A normalised feature n = f * (1 / (sqrt(sum f^2) + eps)) carries at most (C + 6) roundings of relative size u32: C for the sum of
    squares however it is ordered, the products, the square root, the + eps, the reciprocal and the product with it; so |dn| <= (C + 6) u32 |n|.
    The squared difference moves by 2 |n0 - n1| (|dn0| + |dn1|): summed with the non-negative weights that is (C + 6) u32 A.  The difference, its
    square, the weight and the sums over the C channels and the 64 pixels of a block (all terms non-negative: relative errors add) give at most
    (C + 64 + 4) u32 d; the blocks are added in f64 and the result rounded once to f32.  Second-order terms are below 1e-3 of this."""
    return U32 * ((C + 6) * A + (C + 64 + 5) * d)


def _features(seed, B, P, C):
    g = np.random.default_rng(seed)
    f = np.maximum(g.standard_normal((2 * B, P, C)), 0) * g.uniform(0.05, 30, (2 * B, P, 1))     # ReLU outputs, a range of magnitudes per pixel
    f = torch.from_numpy(f).half()
    f[0, 0] = 0                                   # pair 0, pixel 0: an all-zero row in image 0 only
    f[1, 0] = 0
    f[B + 1, 0] = 0                               # pair 1, pixel 0: in both images (the eps path: 0 / (0 + eps))
    f[B + 2, P - 1] = torch.from_numpy(g.uniform(3e4, 65504, C)).half()                          # pair 2, last pixel: a row near the f16 maximum
    return f


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("P", [1, 63, 130])
def test_head_and_finish_vs_f64(dev, C, P):
    """P = 1 and 63: fewer pixels than the 64 of a block (one lane group, one pixel short); 130: two blocks and a last one with 2 pixels."""
    B, eps = 3, 1e-10 * 2.0 ** -6
    f = _features(100 * C + P, B, P, C)
    w = torch.from_numpy(np.abs(np.random.default_rng(C + P).standard_normal(C))).float()
    got, bad = _head(dev, [f], [w], B, eps)
    d, A = _head_f64(f, w, B, eps)
    tol = _head_tol(d, A, C)
    err = (got.to(F64) - d).abs()
    print(f"head C={C} P={P}: d {d.tolist()} |err| {err.tolist()} tol {tol.tolist()}")
    assert torch.isfinite(got).all() and bad.tolist() == [0]
    assert (d[[0, 2]] > 1e-3).all() and (err <= tol).all()
    if P == 1:
        assert d[1] == 0 and got[1] == 0                                               # both rows all zero: 0 / (0 + eps), exactly 0


def test_head_taps_share_a_workspace_and_inf_is_counted(dev):
    """Two taps of different C and P through one workspace (the second tap's section starts after the first's), and planted non-finite features: one inf
    in tap 0, one inf and one NaN in tap 1 are reported per tap; the result of the pair that holds them is then not finite, the others are untouched."""
    B, eps = 3, 1e-10
    f = [_features(7, B, 130, 64), _features(8, B, 63, 512)]
    w = [torch.from_numpy(np.abs(np.random.default_rng(k).standard_normal(c))).float() for k, c in enumerate((64, 512))]
    got, bad = _head(dev, f, w, B, eps)
    d = [_head_f64(fk, wk, B, eps) for fk, wk in zip(f, w)]
    tol = _head_tol(d[0][0], d[0][1], 64) + _head_tol(d[1][0], d[1][1], 512)
    assert bad.tolist() == [0, 0] and ((got.to(F64) - (d[0][0] + d[1][0])).abs() <= tol).all()
    f[0][0, 129, 3] = float("inf")
    f[1][B + 0, 5, 500] = float("inf")
    f[1][0, 62, 0] = float("nan")
    got2, bad2 = _head(dev, f, w, B, eps)
    assert bad2.tolist() == [1, 2] and not torch.isfinite(got2[0]) and got2[1] == got[1]


# ---------------------------------------------------------------------------------------------------------------- engine
def _pairs(z, dev, n=2):
    from tc_light_amd.lpips import pad8_u8
    return pad8_u8(torch.from_numpy(z["source_a"][:n]).to(dev)), pad8_u8(torch.from_numpy(z["edit"][:n]).to(dev))


def _engine_tol(exact, floor):
    """2 x the f16 floor's own error (the margin an f16 path with another summation order gets, as in test_gpu_e2e.py's floor guard) plus, for a pair
    whose floor error happens to vanish, f16's unit round-off at the distance's magnitude."""
    return 2 * np.abs(floor - exact) + U16 * np.abs(exact)


def test_engine_vs_exact_and_floor(dev, engine, golden):
    """2 pairs of 40 x 56 (clip A of the golden file, padded): taps 40x56, 20x28, 10x14, 5x7 and, after an odd floor, 2x3.
    Measured on an MI355X (profiles/lpips_parity.txt): |engine - exact| 5.1e-6 and 3.4e-5, |floor - exact| 1.5e-5 on both, |engine - floor| 2.0e-5 with
    either sign; on the mean of the two 1.5e-5 each.  The engine's f32 sums round a small share of the elements of a layer the other way than the floor's
    f64 sums, and a few layers on the two sets of roundings are independent: the engine's error is another draw of the floor's, not a copy."""
    z = golden("lpips")
    g, e = _pairs(z, dev)
    assert tuple(g.shape) == (2, 40, 56, 3)
    got = engine.distance(g, e).cpu().numpy().astype(np.float64)
    exact, floor = z["a_exact_per"][:2], z["a_floor_per"][:2]
    tol = _engine_tol(exact, floor)
    for i in range(2):
        print(f"pair {i}: engine {got[i]:.8f} exact {exact[i]:.8f} floor {floor[i]:.8f}; |engine - exact| {abs(got[i] - exact[i]):.3e}, "
              f"|floor - exact| {abs(floor[i] - exact[i]):.3e}, |engine - floor| {abs(got[i] - floor[i]):.3e}, tolerance {tol[i]:.3e}")
    m, me, mf = got.mean(), exact.mean(), floor.mean()
    print(f"figure over the 2 pairs: |engine - exact| {abs(m - me):.3e}, |floor - exact| {abs(mf - me):.3e}, |engine - floor| {abs(m - mf):.3e}, "
          f"tolerance {float(_engine_tol(me, mf)):.3e}")
    assert (np.abs(got - exact) <= tol).all()
    assert abs(m - me) <= _engine_tol(me, mf)


def test_engine_identical_frames_are_exactly_zero_and_runs_repeat(dev, engine, golden):
    z = golden("lpips")
    g, e = _pairs(z, dev)
    assert engine.distance(e, e.clone()).cpu().tolist() == [0.0, 0.0]
    a, b = engine.distance(g, e), engine.distance(g, e)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and (a > 0.1).all()


def test_engine_raises_on_non_finite_features(dev, state, golden):
    """A second convolution whose weights are 2^14 times too large overflows f16 at relu1_2: the head counts the inf features and the engine names the tap."""
    from tc_light_amd.lpips import LPIPSEngine
    big = dict(state)
    big["features.2.weight"] = state["features.2.weight"] * 2.0 ** 14
    g, e = _pairs(golden("lpips"), dev, n=1)
    with pytest.raises(FloatingPointError, match="relu1_2"):
        LPIPSEngine(big, dev).distance(g, e)


def test_frame_lpips_end_to_end_vs_golden(dev, engine, golden):
    """4 frames of 36 x 52 (padded to 40 x 56) against a source of 45 x 60 (resized first): the resize, the pad, [:-1] and the mean, clip B of the golden file."""
    from tc_light_amd.evaluate import frame_lpips
    z = golden("lpips")
    exact, floor = z["b_exact_per"], z["b_floor_per"]
    tol, mtol = _engine_tol(exact, floor), _engine_tol(float(z["b_exact_mean"]), float(z["b_floor_mean"]))
    res = {}
    for batch in (1, 3):
        mean, per = frame_lpips(z["edit"], z["source_b"], engine, batch=batch)
        print(f"batch {batch}: frame-lpips {mean:.8f} (exact {float(z['b_exact_mean']):.8f}, floor {float(z['b_floor_mean']):.8f}, tolerance {mtol:.3e}); "
              f"per frame |engine - exact| {np.abs(per - exact).tolist()} tolerance {tol.tolist()}")
        assert per.shape == (3,) and (np.abs(per - exact) <= tol).all() and abs(mean - float(z["b_exact_mean"])) <= mtol
        res[batch] = per
    assert (np.abs(res[1] - res[3]) <= tol).all()
    # clip A (no resize) too, and the one-frame case
    mean, per = frame_lpips(z["edit"], z["source_a"], engine, batch=4)
    assert (np.abs(per - z["a_exact_per"]) <= _engine_tol(z["a_exact_per"], z["a_floor_per"])).all()
    with pytest.raises(ValueError, match="at least 2"):
        frame_lpips(z["edit"][:1], z["source_a"][:1], engine)


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_evaluate_main_with_and_without_lpips(dev, tmp_path, monkeypatch, capsys):
    import importlib.util
    import yaml
    from tc_light_amd.dataparser import write_mjpeg_avi
    from tc_light_amd.evaluate import frame_lpips, read_video_u8
    from tc_light_amd.lpips import LPIPSEngine
    spec = importlib.util.spec_from_file_location("tcl_evaluate_cli", os.path.join(ROOT, "evaluate.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (1, 150, 220, 3), dtype=np.uint8)
    src = np.stack([np.roll(base[0], (k, 2 * k), (0, 1)) for k in range(4)])            # 4 frames, 150 x 220 (resized to the edit size)
    edit = np.clip(src[:, 5:135, 7:205].astype(np.int32) + 20, 0, 255).astype(np.uint8)  # 130 x 198: padded to 136 x 200
    write_mjpeg_avi(str(tmp_path / "output.avi"), edit)
    write_mjpeg_avi(str(tmp_path / "output_gt.avi"), src)
    cfg = {"generation": {"prompt": {"a": "soft light"}}, "models": {"raft": str(tmp_path / "absent.pth"), "lpips_lin": str(tmp_path / "absent_lin.pth")}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    monkeypatch.setenv("TCL_ALLOW_RANDOM_WEIGHTS", "1")
    cli.main(["--output_dir", str(tmp_path)])                                            # allow_random and lpips_lin alone do not switch it on
    off = (tmp_path / "result.txt").read_text()
    out_off = capsys.readouterr().out
    assert [ln.split(": ")[0] for ln in off.splitlines()[1:]] == ["warp-error-ssim"] and "frame-lpips" not in out_off
    assert "not computed here: clip-frame, clip-text, pick-score" in out_off
    scores = cli.main(["--output_dir", str(tmp_path), "--lpips", str(tmp_path / "absent_vgg.pth")])
    on = (tmp_path / "result.txt").read_text()
    out_on = capsys.readouterr().out
    assert [ln.split(": ")[0] for ln in on.splitlines()[1:]] == ["frame-lpips", "warp-error-ssim"]
    e, s = read_video_u8(str(tmp_path / "output.avi")), read_video_u8(str(tmp_path / "output_gt.avi"))
    want, _ = frame_lpips(e, s, LPIPSEngine(R.seeded_state(8), dev))
    assert on.splitlines()[1] == f"frame-lpips: {want:.4f}" and scores["frame-lpips"] == want and want > 0.01
    assert on.replace(f"frame-lpips: {want:.4f}\n", "") == off                           # everything else is what the run without --lpips writes
    assert out_on.replace(f"frame-lpips: {want:.4f}\n", "") == out_off


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(dev, engine):
    L, st = _L()
    x = torch.zeros(2, 4, 4, 96, dtype=torch.float16, device=dev)
    y = torch.full((2, 2, 2, 96), 7.0, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_maxpool2_f16(x, y, 2, 4, 4, 96, st)                                        # C = 96
    one = torch.zeros(2, 1, 1, 512, dtype=torch.float16, device=dev)
    y1 = torch.full((2, 1, 1, 512), 7.0, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_maxpool2_f16(one, y1, 2, 1, 1, 512, st)                                    # a 1 x 1 image into the fourth pool: the pooled size is 0
    ws = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    w = torch.ones(96, dtype=torch.float32, device=dev)
    h_P = torch.tensor([4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_lpips_head(x, w, 1, h_P, 1, 0, 96, 1e-10, ws, st)                          # C = 96
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_lpips_head(x, w, 1, torch.tensor([0], dtype=torch.int32), 1, 0, 64, 1e-10, ws, st)      # no pixels
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_lpips_head(x, w, 1, h_P, 1, 1, 64, 1e-10, ws, st)                          # tap outside the list
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="TCL_EINVAL"):
        L.tcl_lpips_stem_f16(img, w, w, 0.0, 0.0, 0.0, y, 1, 0, 4, st)                   # H < 1
    torch.cuda.synchronize()
    assert (y == 7).all() and (y1 == 7).all() and (ws == 7).all()                        # nothing was written
    a = torch.zeros(1, 40, 56, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="one size"):
        engine.distance(a, torch.zeros(1, 40, 48, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="H, W >= 16"):
        engine.distance(a[:, :8], a[:, :8])
    with pytest.raises(ValueError, match="uint8"):
        engine.distance(a.float(), a.float())
