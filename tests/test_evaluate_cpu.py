"""CPU: the warp-error-ssim restatement (tests/eval_ref.py) on known answers, and the host side of evaluate.py (video lookup, decoding, report)."""
import os
import types

import numpy as np
import pytest
import torch

import eval_ref as R


def _frame(h, w, seed=0):
    return np.random.default_rng(seed).uniform(0, 255, (h, w, 3)).astype(np.float32)


def test_zero_flow_reproduces_the_frame():
    img = _frame(23, 31)
    out = R.remap(img, np.zeros((23, 31, 2), np.float32))
    assert np.array_equal(out, img)


def test_cubic_weights_at_integer_positions_are_a_unit_tap():
    assert np.array_equal(R.cubic_weights(0), np.array([0, 1, 0, 0], np.float32))
    w = R.cubic_weights(np.arange(32))
    assert np.allclose(w.sum(-1), 1, atol=1e-6)


@pytest.mark.parametrize("dx,dy", [(2, 0), (-3, 1), (5, -4), (40, 0)])
def test_integer_shift_gives_exact_shifted_frame(dx, dy):
    H, W = 19, 27
    img = _frame(H, W, seed=1)
    flow = np.zeros((H, W, 2), np.float32)
    flow[..., 0], flow[..., 1] = dx, dy
    out = R.remap(img, flow)
    ref = np.zeros_like(img)
    ys, xs = np.mgrid[0:H, 0:W]
    sy, sx = ys + dy, xs + dx
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    ref[ok] = img[sy[ok], sx[ok]]
    assert np.array_equal(out, ref)


def test_fixed_point_rounds_half_to_even():
    m = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3 + 0.5], np.float32) / np.float32(32)
    ip, fr = R.fixed_point(m)
    assert (ip * 32 + fr).tolist() == [0, 2, 2, 0, -2, 4]
    # a flow of 1/64 px is a tie that rounds to 0 -> the frame itself; 3/64 rounds to 2/32
    img = _frame(9, 11, seed=2)
    f = np.zeros((9, 11, 2), np.float32)
    f[..., 0] = 1 / 64
    assert np.array_equal(R.remap(img, f), img)
    f[..., 0] = 3 / 64
    g = np.zeros_like(f)
    g[..., 0] = 2 / 32
    assert np.array_equal(R.remap(img, f), R.remap(img, g))


def test_u8_cast_truncates_and_wraps():
    assert R.to_u8(np.array([-1.3, 256.7, 300.2, -0.5, 0.99, 255.9], np.float32)).tolist() == [255, 0, 44, 0, 0, 255]


def test_mask_of_consistent_and_inconsistent_flows():
    H, W = 16, 20
    fwd = np.zeros((H, W, 2), np.float32); fwd[..., 0] = 2
    bwd = -fwd
    assert R.consistency_mask(fwd, bwd)[:, 4:-4].all()               # |bwd + fwd(x + bwd)| = 0 away from the border
    assert not R.consistency_mask(fwd, fwd)[:, 4:-4].any()           # |2 fwd| = 4 >= 0.5 * 4 + 0.5


@pytest.mark.parametrize("a,b", [(0, 0), (10, 200), (255, 255), (0, 255), (77, 78)])
def test_ssim_of_constant_planes(a, b):
    x = np.full((12, 15, 3), a, np.uint8)
    y = np.full((12, 15, 3), b, np.uint8)
    expect = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert abs(R.ssim(x, y) - expect) < 1e-12


def test_ssim_of_identical_planes_is_one():
    x = np.random.default_rng(3).integers(0, 256, (20, 30, 3), dtype=np.uint8)
    assert abs(R.ssim(x, x) - 1.0) < 1e-12


def test_warp_pair_with_identity_flows_keeps_everything():
    e0 = np.random.default_rng(4).integers(0, 256, (14, 18, 3), dtype=np.uint8)
    e1 = np.random.default_rng(5).integers(0, 256, (14, 18, 3), dtype=np.uint8)
    z = np.zeros((14, 18, 2), np.float32)
    w, t = R.warp_pair(e0, e1, z, z)
    assert np.array_equal(w, e0) and np.array_equal(t, e1)


# ---------------------------------------------------------------------------------------------------------------- files and report
def _clip(n=3, h=16, w=24, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, (n, 3, h, w)).astype(np.float32))


def test_find_videos_order_and_fallbacks(tmp_path):
    from tc_light_amd.dataparser import save_video
    from tc_light_amd.evaluate import find_videos
    d = str(tmp_path)
    with pytest.raises(FileNotFoundError):
        find_videos(d)
    np.save(os.path.join(d, "output.npy"), np.zeros((2, 8, 8, 3), np.uint8))
    with pytest.raises(FileNotFoundError):                             # an edit but no source
        find_videos(d)
    gt = save_video(_clip(), d, gif=False, post_fix="_gt")
    assert find_videos(d) == (os.path.join(d, "output.npy"), gt)       # output.npy only as the last resort
    out = save_video(_clip(seed=1), d, gif=False)
    assert find_videos(d)[0] == out and not out.endswith(".npy")
    opt = save_video(_clip(seed=2), d, gif=False, post_fix="_opt")
    assert find_videos(d)[0] == opt                                    # output_opt before output
    for stem in ("output_opt", "output_gt"):                           # .mp4 before .avi for each stem
        open(os.path.join(d, stem + ".mp4"), "wb").close()
    assert find_videos(d) == (os.path.join(d, "output_opt.mp4"), os.path.join(d, "output_gt.mp4"))


def test_read_video_u8_is_exact(tmp_path):
    from tc_light_amd.dataparser import read_mjpeg_avi, write_mjpeg_avi
    from tc_light_amd.evaluate import read_video_u8
    fr = np.random.default_rng(6).integers(0, 256, (3, 16, 24, 3), dtype=np.uint8)
    np.save(tmp_path / "output.npy", fr)
    got = read_video_u8(str(tmp_path / "output.npy"))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), fr)
    write_mjpeg_avi(str(tmp_path / "output.avi"), fr)
    got = read_video_u8(str(tmp_path / "output.avi"))
    assert got.dtype == torch.uint8 and torch.equal(got, read_mjpeg_avi(str(tmp_path / "output.avi")))


def test_format_results_and_cost_keys(tmp_path):
    from tc_light_amd.config_utils import _wrap, save_config
    from tc_light_amd.evaluate import cost_scores, format_results, video_name
    import yaml
    cfg = _wrap({"input_path": "data/videos/kitchen/clip.mp4", "generation": {"prompt": {"a": "warm light"}}, "sec_per_frame": 0.25,
                 "max_memory_allocated": 1234.5, "total_number_of_frames": 30, "total_time": 7.5})
    save_config(cfg, str(tmp_path))
    loaded = _wrap(yaml.safe_load(open(tmp_path / "config.yaml")))
    scores = {"warp-error-ssim": 0.912345, "pick-score": 21.123456}
    scores.update(cost_scores(loaded, 64, 36))
    text = format_results(video_name(loaded), "warm light", scores)
    lines = text.splitlines()
    assert lines[0] == "kitchen - warm light"
    assert lines[1:] == ["pick-score: 21.1235", "warp-error-ssim: 91.23", "z_fps: 4.0000", "z_max_memory_allocated(M): 1234.5000",
                         "z_resolution: 48.0000", "z_total_frames: 30.0000", "z_total_time(s): 7.5000"]
    assert video_name(_wrap({"generation": {}})) == "unknown_video"
    with pytest.raises(KeyError):
        cost_scores(_wrap({}), 64, 36)


def test_warp_ssim_refuses_short_clips_and_small_sizes():
    from tc_light_amd.evaluate import warp_ssim
    eng = types.SimpleNamespace(dev=torch.device("cpu"))
    one = np.zeros((1, 128, 128, 3), np.uint8)
    with pytest.raises(ValueError):
        warp_ssim(one, one, eng)
    small = np.zeros((3, 120, 256, 3), np.uint8)                      # pads to 120: H / 64 < 2
    with pytest.raises(ValueError):
        warp_ssim(small, small, eng)
