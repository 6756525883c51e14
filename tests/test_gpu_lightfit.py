"""GPU: tcl_light_fit_u8 (csrc/lightfit.hip) and evaluate.py --light against the float64 restatement tests/lightfit_refs.py.

Every sum is held to the bound the header's float sequence and summation order allow (lightfit_refs' docstring derives it: Sum(w m) times
gamma32(77) + gamma64(9 + nb); Sum w exactly), two runs to the same bits, and the fitted angle to the restatement's own within the angle error those
bounds imply -- angle_bound_deg computes it per frame; over the planted frames used here it is 2.5e-3 to 2.8e-3 degrees at every size (37x53,
5x2051, 64x2048; printed by test_planted_angles), plus 1e-9 for the two f64 solves (Cramer's rule there, LU here)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import lightfit_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0

# name -> (N, H, W, planted angles): 37x53 is odd and smaller than one block's span of 16384 pixels; 1x1; 5x2051 = 10255 pixels ends inside a
# 16-pixel chunk and inside the block (byte loads); 64x2048 = 8 blocks per frame (16 B loads, the workspace and the finish order)
CASES = {"odd_37x53": (3, 37, 53, (37.0, 200.0, 315.0)), "one_pixel": (1, 1, 1, (0.0,)), "tails_5x2051": (2, 5, 2051, (0.0, 90.0)),
         "blocks_64x2048": (2, 64, 2048, (37.0, 315.0)), "clipped_frame": (2, 37, 53, (90.0, 90.0))}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _inputs(name):
    N, H, W, angles = CASES[name]
    E, S = R.planted(N, H, W, angles, seed=len(name))
    rng = np.random.default_rng(17)
    if name == "clipped_frame":
        E[1] = 255                                                           # frame 1: every pixel clipped in E
    elif name != "one_pixel":
        drop = rng.random((N, 1, H, W)) < 0.03                               # a sprinkle of clipped pixels in either clip, and of colour
        E = np.where(drop, rng.choice([0, 1, 254, 255], (N, 1, H, W)).astype(np.uint8), E)
        S = np.where(np.roll(drop, 3, axis=-1), rng.choice([0, 255], (N, 1, H, W)).astype(np.uint8), S)
        E[:, 0] = np.clip(E[:, 0].astype(np.int32) + rng.integers(-2, 3, (N, H, W)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(E), np.ascontiguousarray(S)


_CACHE = {}


def _case(name, dev):
    """(E, S on the device, reference sums, bounds, the kernel's sums as numpy) -- computed once per case and shared, never modified."""
    if name not in _CACHE:
        from tc_light_amd.lightfit import light_sums
        E, S = _inputs(name)
        sums, bound = R.sums_ref(E, S)
        e, s = torch.from_numpy(E).to(dev), torch.from_numpy(S).to(dev)
        got = light_sums(e, s).cpu().numpy()
        for a in (sums, bound, got):
            a.setflags(write=False)
        _CACHE[name] = (e, s, sums, bound, got)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_sums_within_their_bounds(dev, name):
    _, _, sums, bound, got = _case(name, dev)
    assert got.shape == sums.shape and got.dtype == np.float64 and np.isfinite(got).all()
    err = np.abs(got - sums)
    for k, term in enumerate(("w", "wu", "wv", "wuu", "wuv", "wvv", "wr", "wru", "wrv", "wrr")):
        print(f"{name} S{term}: max |err| {err[:, k].max():.3e}, bound {bound[:, k].max():.3e}, |sum| {np.abs(sums[:, k]).max():.6e}")
    assert (got[:, 0] == sums[:, 0]).all(), "Sum w is exact: the same pixels clip"
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    if name == "clipped_frame":
        assert (got[1] == 0).all() and got[0, 0] == 37 * 53
    if name == "one_pixel":
        assert got[0, 0] == 1.0 and got[0, 1] == 0.0 and got[0, 2] == 0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_runs_are_bit_equal(dev, name):
    from tc_light_amd.lightfit import light_sums
    e, s, _, _, got = _case(name, dev)
    again = light_sums(e, s).cpu().numpy()
    assert again.tobytes() == got.tobytes()
    if name == "tails_5x2051":                                               # a base that is not 16 B aligned takes the same path: the same bits
        buf = torch.empty(e.numel() + 1, dtype=torch.uint8, device=dev)
        buf[1:].copy_(e.reshape(-1))
        assert light_sums(buf[1:].view(e.shape), s).cpu().numpy().tobytes() == got.tobytes()
    if name == "blocks_64x2048":                                             # ... and here the byte loads must give the bits of the 16 B loads
        buf = torch.empty(s.numel() + 3, dtype=torch.uint8, device=dev)
        buf[3:].copy_(s.reshape(-1))
        assert light_sums(e, buf[3:].view(s.shape)).cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("name", ["odd_37x53", "tails_5x2051", "blocks_64x2048"])
def test_planted_angles(dev, name):
    from tc_light_amd.lightfit import figures
    _, _, sums, bound, got = _case(name, dev)
    angles = CASES[name][3]
    follow, contrast, frames = figures(got, angles)
    for f, row, b, want in zip(frames, sums, bound, angles):
        ok, ang, con, r2 = R.solve_ref(row)
        tol = R.angle_bound_deg(row, b)
        print(f"{name}: planted {want}, reference {ang:.6f}, kernel {f['angle']:.6f}, implied angle bound {tol:.3e} deg")
        assert ok and f["estimate"]
        assert tol < 0.05 and R.angle_diff(f["angle"], ang) <= tol + 1e-9
        assert R.angle_diff(ang, want) <= 2.0                                # the inputs' own condition (test_lightfit_refs_cpu.py)
    rf, rc = R.figures_ref(sums, angles)
    assert abs(follow - rf) <= 1e-3 and abs(contrast - rc) <= 1e-3 * rc and follow > 0.999


def test_clipped_frame_counts_as_no_estimate(dev):
    from tc_light_amd.lightfit import figures
    got = _case("clipped_frame", dev)[4]
    follow, contrast, frames = figures(got, [90.0, 90.0])
    assert [f["estimate"] for f in frames] == [True, False] and frames[1]["cos"] == 0.0
    assert abs(follow - frames[0]["cos"] / 2) < 1e-15 and 0.49 < follow <= 0.5


def test_bad_arguments_are_refused_and_write_nothing(dev):
    from tc_light_amd.lib import lib, stream
    L = lib()
    e = torch.full((2, 3, 8, 8), 100, dtype=torch.uint8, device=dev)
    s = torch.full((2, 3, 8, 8), 90, dtype=torch.uint8, device=dev)
    out = torch.full((2, 10), SENTINEL, dtype=torch.float64, device=dev)
    ws = torch.full((64,), SENTINEL, dtype=torch.float64, device=dev)
    assert L.tcl_light_fit_workspace_bytes(2, 8, 8) == 2 * 10 * 8 and L.tcl_light_fit_workspace_bytes(60, 720, 1280) == 60 * 57 * 10 * 8
    bad = [(e, s, 0, 8, 8, out, ws), (e, s, -1, 8, 8, out, ws), (e, s, 65536, 8, 8, out, ws), (e, s, 2, 0, 8, out, ws), (e, s, 2, 8, -3, out, ws),
           (e, s, 2, 65536, 32768, out, ws), (None, s, 2, 8, 8, out, ws), (e, None, 2, 8, 8, out, ws), (e, s, 2, 8, 8, None, ws),
           (e, s, 2, 8, 8, out, None)]
    for args in bad:
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_light_fit_u8(*args, stream())
        assert L.tcl_light_fit_workspace_bytes(*args[2:5]) == 0 or args[2:5] == (2, 8, 8)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (ws == SENTINEL).all()
    L.tcl_light_fit_u8(e, s, 2, 8, 8, out, ws, stream())                      # the same buffers, good arguments: now it writes
    assert (out[:, 0] == 64).all()


def test_evaluate_cli_light(dev, tmp_path, capsys):
    """evaluate.py --light on a synthetic run directory: 3 frames, a two-keyframe path.  128x128, not 64x64: RAFT's size check (H/64 >= 2), which
    warp-error-ssim runs under, refuses anything smaller.  result.txt gains exactly the two lines and light_follow.json has 3 entries; without
    --light the file is what the code path before this figure writes (format_results over warp-error-ssim alone)."""
    import json
    import yaml
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import evaluate as top
    from tc_light_amd.evaluate import format_results, warp_ssim
    from tc_light_amd.raft import RAFTEngine, seeded_state_dict
    E, S = R.planted(3, 128, 128, (0.0, 90.0, 180.0), seed=1)
    np.save(tmp_path / "output.npy", E)
    np.save(tmp_path / "output_gt.npy", S)
    cfg = {"generation": {"prompt": {"a": "soft light"}, "light_path": [[0, 0], [1, 180]]}, "models": {"allow_random": True}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    top.main(["--output_dir", str(tmp_path)])
    before = (tmp_path / "result.txt").read_text()
    assert not (tmp_path / "light_follow.json").exists()
    score, _ = warp_ssim(E.transpose(0, 2, 3, 1), S.transpose(0, 2, 3, 1), RAFTEngine(seeded_state_dict(5), dev))
    assert before == format_results("unknown_video", "soft light", {"warp-error-ssim": score})
    scores = top.main(["--output_dir", str(tmp_path), "--light"])
    after = (tmp_path / "result.txt").read_text()
    lines, old = after.splitlines(), before.splitlines()
    assert lines == [old[0], f"light-contrast: {scores['light-contrast']:.4f}", f"light-follow: {scores['light-follow']:.4f}"] + old[1:]
    frames = json.loads((tmp_path / "light_follow.json").read_text())
    assert len(frames) == 3 and [f["wanted"] for f in frames] == [0.0, 90.0, 180.0]
    assert all(f["estimate"] and R.angle_diff(f["angle"], f["wanted"]) <= 2.0 and 0.9 < f["r2"] <= 1.0 for f in frames)
    assert set(frames[0]) == {"frame", "wanted", "angle", "contrast", "r2", "estimate", "cos"}
    assert scores["light-follow"] > 0.999 and abs(scores["light-contrast"] - R.AMPLITUDE) < 0.05 * R.AMPLITUDE
    flipped = top.main(["--output_dir", str(tmp_path), "--light", "--light_path", "[[0,180],[1,360]]"])       # the override wins over the config
    assert flipped["light-follow"] < -0.999
    capsys.readouterr()
