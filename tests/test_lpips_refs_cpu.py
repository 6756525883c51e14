"""CPU: the float64 restatement of frame-lpips (tests/lpips_refs.py) pinned independently of itself, and the host side of the feature: the padder, the
`[:-1]` rule, the loader, the settings, the report and the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lpips_refs as R

F64 = torch.float64


@pytest.fixture(scope="module")
def state():
    return R.seeded_state(8)


def _images(seed, n, h, w):
    """uint8-valued [n,3,h,w] float64 images whose border pixels are far from the scaling layer's shift colour (about 0)."""
    g = np.random.default_rng(seed)
    x = g.integers(0, 256, (n, 3, h, w)).astype(np.float64)
    x[:, :, 0, :] = 255
    x[:, :, :, -1] = 200
    return torch.from_numpy(x)


# ---------------------------------------------------------------------------------------------------------------- the refs against direct loops
def _conv3_relu_loops(x, w, b):
    """x [C,H,W], w [O,C,3,3], b [O] numpy float64 -> relu(conv, zero padding 1) by loops over the pixels and the taps."""
    C, H, W = x.shape
    y = np.zeros((w.shape[0], H, W))
    for i in range(H):
        for j in range(W):
            acc = b.copy()
            for ky in range(3):
                for kx in range(3):
                    ii, jj = i + ky - 1, j + kx - 1
                    if 0 <= ii < H and 0 <= jj < W:
                        acc = acc + w[:, :, ky, kx] @ x[:, ii, jj]
            y[:, i, j] = np.maximum(acc, 0)
    return y


def _tap0_loops(img, sd):
    x = np.empty_like(img)
    for c in range(3):
        x[c] = (img[c] - R.SHIFT[c]) / R.SCALE[c]                                    # the scaling layer; the zero padding below is of THIS image
    t = _conv3_relu_loops(x, sd["features.0.weight"].double().numpy(), sd["features.0.bias"].double().numpy())
    return _conv3_relu_loops(t, sd["features.2.weight"].double().numpy(), sd["features.2.bias"].double().numpy())


def test_refs_stem_tap_head_vs_numpy_loops(state):
    x = _images(1, 2, 5, 6)
    f = [_tap0_loops(x[i].numpy(), state) for i in range(2)]
    got = [R.taps(x[i:i + 1], state, n_taps=1)[0][0].numpy() for i in range(2)]
    for a, b in zip(f, got):
        assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max()
    w = state["lin0.model.1.weight"].reshape(-1).double().numpy()
    d = 0.0
    for i in range(5):
        for j in range(6):
            a, b = f[0][:, i, j], f[1][:, i, j]
            na, nb = a / (np.sqrt((a * a).sum()) + 1e-10), b / (np.sqrt((b * b).sum()) + 1e-10)
            d += float((w * (na - nb) ** 2).sum())
    d /= 30
    ref = R.head(torch.from_numpy(got[0])[None], torch.from_numpy(got[1])[None], torch.from_numpy(w)).item()
    assert d > 1e-3 and abs(ref - d) <= 1e-12 * d


def test_refs_identity_symmetry_and_tap_shapes(state):
    x = _images(2, 2, 21, 37)
    assert [tuple(t.shape[1:]) for t in R.taps(x[:1], state)] == [(64, 21, 37), (128, 10, 18), (256, 5, 9), (512, 2, 4), (512, 1, 2)]
    assert R.distance(x, x, state).tolist() == [0.0, 0.0]
    assert R.distance(x, x, state, s=2.0 ** -6, f16=True).tolist() == [0.0, 0.0]
    d01, d10 = R.distance(x[:1], x[1:], state), R.distance(x[1:], x[:1], state)
    assert d01.item() > 0.05 and d01.item() == d10.item()


def test_refs_power_of_two_input_scale_leaves_the_result_unchanged(state):
    """relu(conv(s x) + s b) = s relu(conv(x) + b) and max-pooling commutes with s > 0, so with the biases and eps scaled by s every normalised feature
    is the same number; for a power of two the scaling is exact in binary floating point, so float64 gives the same BITS."""
    x = _images(3, 2, 16, 24)
    d1 = R.distance(x[:1], x[1:], state, s=1.0)
    for s in (2.0 ** -6, 2.0 ** -10, 4.0):
        t1, ts = R.taps(x[:1], state, 1.0), R.taps(x[:1], state, s)
        for a, b in zip(t1, ts):
            assert torch.equal(a * s, b)
        assert R.distance(x[:1], x[1:], state, s=s).item() == d1.item()
    # and the biases do matter to it: leaving them unscaled changes the figure
    unscaled = {k: (v / 2.0 ** -6 if k.endswith(".bias") else v) for k, v in state.items()}
    assert abs(R.distance(x[:1], x[1:], unscaled, s=2.0 ** -6).item() - d1.item()) > 1e-6 * d1.item()


def test_border_rule_padding_after_scaling(state):
    """Conv2d's zero padding is of the scaled image.  Padding the 0..255 image with 0 and scaling afterwards puts -shift / scale outside the frame:
    the two agree in the interior and differ on every border pixel."""
    import torch.nn.functional as F
    x = _images(4, 1, 7, 9)
    w, b = state["features.0.weight"].double(), state["features.0.bias"].double()
    after = F.conv2d(R.scaling_layer(x), w, b, padding=1)                              # what the refs (and LPIPS) do
    before = F.conv2d(R.scaling_layer(F.pad(x, [1, 1, 1, 1])), w, b)
    assert torch.allclose(after[..., 1:-1, 1:-1], before[..., 1:-1, 1:-1], rtol=0, atol=1e-9)
    border = torch.ones(7, 9, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    diff = (after - before).abs().amax(1)[0]
    assert (diff[border] > 1e-3).all()
    # the refs' own first layer is the `after` one: an identity second convolution (centre tap 1 on the diagonal, no bias) hands it through
    eye = torch.zeros(64, 64, 3, 3)
    eye[torch.arange(64), torch.arange(64), 1, 1] = 1
    through = R.taps(x, {**state, "features.2.weight": eye, "features.2.bias": torch.zeros(64)}, n_taps=1)[0]
    assert torch.equal(through, torch.relu(after))


# ---------------------------------------------------------------------------------------------------------------- the padder, [:-1]
@pytest.mark.parametrize("H,W,amounts", [(36, 52, (2, 2, 2, 2)), (37, 53, (1, 2, 1, 2)), (40, 56, (0, 0, 0, 0)), (33, 49, (3, 4, 3, 4))])
def test_padder_vs_hand_written(H, W, amounts):
    from tc_light_amd.flow_core import pad8
    from tc_light_amd.hostlogic import pad8_amounts
    from tc_light_amd.lpips import pad8_u8
    l, r, t, b = amounts
    assert pad8_amounts(H, W) == amounts
    g = np.random.default_rng(H)
    x = g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    want = np.empty((2, H + t + b, W + l + r, 3), np.uint8)
    for i in range(want.shape[1]):
        for j in range(want.shape[2]):
            want[:, i, j] = x[:, min(max(i - t, 0), H - 1), min(max(j - l, 0), W - 1)]
    assert want.shape[1] % 8 == 0 and want.shape[2] % 8 == 0 and want.shape[1] - H < 8 and want.shape[2] - W < 8
    got = pad8_u8(torch.from_numpy(x))
    assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.numpy(), want)
    nchw = torch.from_numpy(x).permute(0, 3, 1, 2).double()
    assert np.array_equal(R.pad8(nchw).permute(0, 2, 3, 1).numpy(), want.astype(np.float64))
    ref, pad = pad8(nchw)
    assert tuple(pad) == amounts and np.array_equal(ref.permute(0, 2, 3, 1).numpy(), want.astype(np.float64))


class _RefEngine:
    """tc_light_amd.evaluate.frame_lpips's engine argument, answered by the float64 refs on the CPU: the host path is then testable without a GPU."""
    dev = torch.device("cpu")

    def __init__(self, state):
        self.state, self.calls = state, []

    def distance(self, a, b):
        assert a.dtype == torch.uint8 and a.shape == b.shape and a.shape[1] % 8 == 0 and a.shape[2] % 8 == 0
        self.calls.append(a.shape[0])
        return R.distance(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), self.state).float()


def test_frame_lpips_leaves_the_last_frame_out(state):
    from tc_light_amd.evaluate import frame_lpips
    g = np.random.default_rng(5)
    edit = g.integers(0, 256, (4, 17, 20, 3), dtype=np.uint8)
    src = g.integers(0, 256, (4, 17, 20, 3), dtype=np.uint8)
    eng = _RefEngine(state)
    mean, per = frame_lpips(edit, src, eng, batch=2)
    assert per.shape == (3,) and per.dtype == np.float64 and eng.calls == [2, 1] and mean == float(np.mean(per))
    rmean, rper = R.frame_lpips(edit, src, state)
    assert np.abs(per - rper).max() <= 1e-6 * rper.max() and abs(mean - rmean) <= 1e-6 * rmean
    other = edit.copy()
    other[-1] = 255 - other[-1]                                                        # the last relit frame is never looked at
    assert np.array_equal(frame_lpips(other, src[:3], _RefEngine(state))[1], per)      # nor is a last source frame needed
    with pytest.raises(ValueError, match="at least 2"):
        frame_lpips(edit[:1], src[:1], eng)
    with pytest.raises(ValueError, match="at least 2"):
        R.frame_lpips(edit[:1], src[:1], state)
    with pytest.raises(ValueError):
        frame_lpips(edit, src[:2], eng)


def test_frame_lpips_host_path_vs_golden(golden, state):
    """Resize of a source of another size, pad, [:-1] and the mean, against tests/golden/lpips.npz (clip B; exact mode)."""
    from tc_light_amd.evaluate import frame_lpips
    z = golden("lpips")
    assert int(z["seed"]) == 8 and float(z["bias_std"]) == 0.05
    mean, per = frame_lpips(z["edit"], z["source_b"], _RefEngine(state), batch=3)
    assert np.abs(per - z["b_exact_per"]).max() <= 1e-6 and abs(mean - float(z["b_exact_mean"])) <= 1e-6
    # the floor of the golden file is the refs' too (one pair of clip A: keeps the test short)
    f = R.frame_lpips(z["edit"][:2], z["source_a"][:2], state, s=float(z["input_scale"]), f16=True)[1]
    assert f[0] == z["a_floor_per"][0]


# ---------------------------------------------------------------------------------------------------------------- the loader
def _zeros(shapes):
    return {k: torch.zeros(1).expand(s) for k, s in shapes.items()}                    # stride-0 views: the files stay a few kB


def test_loader_reads_a_complete_pair_and_names_what_is_wrong(tmp_path, monkeypatch):
    from tc_light_amd import lpips as LP
    from tc_light_amd.model_utils import load_lpips_state
    monkeypatch.delenv("TCL_ALLOW_RANDOM_WEIGHTS", raising=False)
    vgg, lin = _zeros(LP.vgg_param_shapes()), _zeros(LP.lin_param_shapes())
    vp, lp = str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")
    torch.save({**vgg, "classifier.0.weight": torch.zeros(2, 2)}, vp)
    torch.save(lin, lp)
    sd = load_lpips_state(vp, lp)
    assert set(sd) == set(vgg) | set(lin) and all(tuple(sd[k].shape) == tuple(s) for k, s in {**LP.vgg_param_shapes(), **LP.lin_param_shapes()}.items())
    assert all(v.dtype == torch.float32 and not v.any() for v in sd.values())
    bad = str(tmp_path / "bad.pth")
    for k in vgg:
        torch.save({q: v for q, v in vgg.items() if q != k}, bad)
        with pytest.raises(KeyError, match=k.replace(".", r"\.")):
            load_lpips_state(bad, lp)
        torch.save({**vgg, k: torch.zeros(1).expand(tuple(vgg[k].shape) + (1,))}, bad)
        with pytest.raises(KeyError, match=k.replace(".", r"\.")):
            load_lpips_state(bad, lp)
    for k in lin:
        torch.save({q: v for q, v in lin.items() if q != k}, bad)
        with pytest.raises(KeyError, match=k.replace(".", r"\.")):
            load_lpips_state(vp, bad)
        torch.save({**lin, k: torch.zeros(1).expand(lin[k].shape[1], 1, 1, 1)}, bad)
        with pytest.raises(KeyError, match=k.replace(".", r"\.")):
            load_lpips_state(vp, bad)
    with pytest.raises(KeyError, match="lin0"):
        LP.check_state({k: v for k, v in sd.items() if k != "lin0.model.1.weight"})


def test_loader_missing_file_and_stand_ins(tmp_path, monkeypatch):
    from tc_light_amd import lpips as LP
    from tc_light_amd.model_utils import allow_random, load_lpips_state
    monkeypatch.delenv("TCL_ALLOW_RANDOM_WEIGHTS", raising=False)
    lp = str(tmp_path / "lin.pth")
    torch.save(_zeros(LP.lin_param_shapes()), lp)
    with pytest.raises(FileNotFoundError):
        load_lpips_state(str(tmp_path / "absent.pth"), lp)
    with pytest.raises(FileNotFoundError):
        load_lpips_state(None, None)
    with pytest.warns(UserWarning, match="stand-ins"):
        sd = load_lpips_state(str(tmp_path / "absent.pth"), lp, allow=True)
    ref = LP.seeded_state(8)
    assert torch.equal(sd["features.28.weight"], ref["features.28.weight"]) and not sd["lin3.model.1.weight"].any()      # the file that exists is read
    monkeypatch.setenv("TCL_ALLOW_RANDOM_WEIGHTS", "1")
    with pytest.warns(UserWarning):
        sd = load_lpips_state(None, None, allow=allow_random({}))
    assert all(torch.equal(sd[k], ref[k]) for k in ref)
    assert all((ref[f"lin{k}.model.1.weight"] >= 0).all() for k in range(5))
    assert all(torch.equal(v, v.half().float()) for k, v in ref.items() if k.startswith("features."))


def test_lpips_settings_precedence():
    from tc_light_amd.evaluate import lpips_settings
    m = {"lpips_vgg": "cfg_vgg.pth", "lpips_lin": "cfg_lin.pth", "allow_random": True}
    assert lpips_settings(m) == ("cfg_vgg.pth", "cfg_lin.pth")
    assert lpips_settings(m, "arg_vgg.pth") == ("arg_vgg.pth", "cfg_lin.pth")
    assert lpips_settings(m, "arg_vgg.pth", "arg_lin.pth") == ("arg_vgg.pth", "arg_lin.pth")
    assert lpips_settings({}, "arg_vgg.pth") == ("arg_vgg.pth", None)
    for off in ({}, None, {"allow_random": True}, {"lpips_vgg": "", "lpips_lin": "cfg_lin.pth"}):
        assert lpips_settings(off) == (None, None)                                     # allow_random alone never switches it on; nor does lpips_lin
    assert lpips_settings({}, None, "arg_lin.pth") == (None, None)


def test_format_results_gains_the_line_only_with_the_score():
    from tc_light_amd import evaluate as E
    scores = {"warp-error-ssim": 0.91234, "clip-frame": 0.98765, "clip-text": 0.3, "pick-score": 21.5}
    base = E.format_results("clip_a", "soft light", scores)
    assert base == "clip_a - soft light\nclip-frame: 0.9877\nclip-text: 0.3000\npick-score: 21.5000\nwarp-error-ssim: 91.23\n"
    with_l = E.format_results("clip_a", "soft light", {**scores, "frame-lpips": 0.42662})
    assert with_l.splitlines() == ["clip_a - soft light", "clip-frame: 0.9877", "clip-text: 0.3000", "frame-lpips: 0.4266", "pick-score: 21.5000",
                                   "warp-error-ssim: 91.23"]
    assert with_l.replace("frame-lpips: 0.4266\n", "") == base
    assert "frame-lpips" not in E.NOT_COMPUTED and "frame-lpips" not in E.not_computed(False, False)


def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH, parse_header
    if not os.path.exists(LIB_PATH):
        g.build()
    sig = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("tcl_lpips_stem_f16", 11), ("tcl_maxpool2_f16", 7), ("tcl_lpips_workspace_bytes", 3), ("tcl_lpips_head", 10),
                        ("tcl_lpips_finish", 7)):
        assert name in sig and len(sig[name][1]) == nargs and hasattr(dll, name), name
    assert sig["tcl_lpips_workspace_bytes"][0] is ctypes.c_size_t


def test_workspace_size_and_refusals_without_a_launch():
    """The host-side answers of the C ABI: they touch no device memory, so they are checked here too."""
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        g.build()
    L = lib()
    blocks = lambda p: -(-p // 64)
    assert L.tcl_lpips_workspace_bytes(3, 40, 56) == 3 * 8 * (blocks(40 * 56) + blocks(20 * 28) + blocks(10 * 14) + blocks(5 * 7) + blocks(2 * 3))
    assert L.tcl_lpips_workspace_bytes(1, 720, 1280) == 8 * (14400 + 3600 + 900 + 225 + blocks(45 * 80))
    for B, H, W in ((0, 40, 56), (1, 15, 56), (1, 40, 15), (1, 0, 8), (70000, 40, 56)):
        assert L.tcl_lpips_workspace_bytes(B, H, W) == 0
    assert L.tcl_lpips_workspace_bytes(1, 16, 16) == 8 * (4 + 1 + 1 + 1 + 1)
