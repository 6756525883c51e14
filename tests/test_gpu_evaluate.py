"""GPU: warp-error-ssim (csrc/evaluate.hip, tc_light_amd/evaluate.py, evaluate.py) against its CPU restatement tests/eval_ref.py: the warp + mask
planes, the SSIM kernel, determinism, the whole metric with the engine's own RAFT flows, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _smooth(rng, shape, cells):
    """A smooth random field [*shape] (bilinear up-sampling of a coarse grid)."""
    H, W = shape[-2:]
    g = torch.from_numpy(rng.standard_normal((1, shape[0], cells, cells)).astype(np.float32))
    return torch.nn.functional.interpolate(g, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()


def _pair_inputs(H, W, seed):
    """Two edit frames and a (fut, past) pair of flows whose forward-backward check passes on part of the frame, with vectors that point outside
    the frame and fractions on exact 1/64 ties (the rint half-to-even case of the 1/32-pixel grid)."""
    rng = np.random.default_rng(seed)
    edit = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    base = 6 * _smooth(rng, (2, H, W), 6)
    bwd = base + 0.3 * rng.standard_normal((2, H, W)).astype(np.float32)
    fwd = -base + 0.6 * _smooth(rng, (2, H, W), 9) + 0.3 * rng.standard_normal((2, H, W)).astype(np.float32)
    for f in (fwd, bwd):
        tie = rng.random((H, W)) < 0.05                                 # k / 64 with k odd: m * 32 ends in .5
        k = 2 * rng.integers(-200, 200, (2, H, W)) + 1
        f[:, tie] = (k[:, tie] / 64.0).astype(np.float32)
        far = rng.random((H, W)) < 0.01                                 # well outside the frame
        f[:, far] = rng.choice([-1, 1], (2, int(far.sum()))) * rng.uniform(W, 3 * W, (2, int(far.sum())))
    fut = np.zeros((2, 2, H, W), np.float32); past = np.zeros_like(fut)
    fut[0], past[1] = fwd, bwd
    return edit, fut, past


@pytest.mark.parametrize("H,W", [(131, 257), (720, 1280)])
def test_warp_mask_planes_vs_ref(dev, H, W):
    from tc_light_amd.evaluate import warp_mask_planes
    edit, fut, past = _pair_inputs(H, W, seed=H)
    w, t = warp_mask_planes(torch.from_numpy(edit).to(dev), torch.from_numpy(fut).to(dev), torch.from_numpy(past).to(dev), 0, 1)
    w, t = w[0].cpu().numpy(), t[0].cpu().numpy()
    rw, rt, wf, lhs, rhs = R.warp_pair(edit[0], edit[1], fut[0].transpose(1, 2, 0), past[1].transpose(1, 2, 0), return_float=True)
    m = lhs < rhs
    assert 0.05 < m.mean() < 0.95, f"the mask should be mixed, kept {m.mean():.3f}"
    bad = (w != rw) | (t != rt)
    assert bad.mean() <= 1e-4, f"{bad.sum()} of {bad.size} u8 elements differ"
    ys, xs, cs = np.nonzero(bad)
    near_int = np.abs(wf[ys, xs, cs] - np.rint(wf[ys, xs, cs])) < 1e-3
    tie = np.abs(lhs[ys, xs] - rhs[ys, xs]) < 1e-4
    assert (near_int | tie).all(), f"unexplained mismatches at {list(zip(ys[~(near_int | tie)], xs[~(near_int | tie)]))[:5]}"


@pytest.mark.parametrize("case", ["random", "all255", "zero_vs_255", "odd_small", "odd_large"])
def test_ssim_kernel_vs_ref(dev, case):
    from tc_light_amd.evaluate import ssim_u8
    rng = np.random.default_rng(7)
    shape = {"odd_small": (2, 7, 9, 3), "odd_large": (2, 133, 71, 3)}.get(case, (3, 131, 257, 3))
    if case == "all255":
        x = np.full(shape, 255, np.uint8); y = x.copy()
    elif case == "zero_vs_255":
        x = np.zeros(shape, np.uint8); y = np.full(shape, 255, np.uint8)
    else:
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        y = np.clip(x.astype(np.int32) + rng.integers(-40, 40, shape), 0, 255).astype(np.uint8)
        y[0] = rng.integers(0, 256, shape[1:], dtype=np.uint8)                 # one unrelated pair
    got = ssim_u8(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)).cpu().numpy()
    ref = np.array([R.ssim(a, b) for a, b in zip(x, y)])
    assert np.abs(got - ref).max() <= 1e-6, (got, ref)


def test_warp_ssim_from_flows_is_deterministic(dev):
    from tc_light_amd.evaluate import warp_ssim_from_flows
    rng = np.random.default_rng(9)
    N, H, W = 6, 144, 200
    edit = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(dev)
    fut = torch.from_numpy(3 * rng.standard_normal((N, 2, H, W)).astype(np.float32)).to(dev)
    past = torch.from_numpy(3 * rng.standard_normal((N, 2, H, W)).astype(np.float32)).to(dev)
    m1, p1 = warp_ssim_from_flows(edit, fut, past, batch=2)
    m2, p2 = warp_ssim_from_flows(edit, fut, past, batch=2)
    assert p1.tobytes() == p2.tobytes() and m1 == m2
    m3, p3 = warp_ssim_from_flows(edit, fut, past, batch=5)                   # the batch split does not change a pair's score
    assert p3.tobytes() == p1.tobytes()


def _u8(x):
    return (x.permute(0, 2, 3, 1) * 255).round().clamp(0, 255).to(torch.uint8)


def test_warp_ssim_whole_metric_vs_ref(dev):
    import synth
    from tc_light_amd.evaluate import warp_ssim
    from tc_light_amd.raft import RAFTEngine, estimate_flows_raft, seeded_state_dict
    d = synth.video_clip(8, 192, 256, seed=4)
    src, edit = _u8(d["frames"]), _u8(d["edited"])
    eng = RAFTEngine(seeded_state_dict(), dev)
    score, per = warp_ssim(edit, src, eng, batch=4)
    fut, past = estimate_flows_raft(eng, src.permute(0, 3, 1, 2).float().to(dev), batch=4)
    ref, rper = R.warp_ssim_from_flows(edit.numpy(), fut.cpu().numpy(), past.cpu().numpy())
    assert len(per) == 7 and np.isfinite(per).all()
    assert abs(score - ref) <= 1e-4, (score, ref, per, rper)


def test_evaluate_cli(dev, tmp_path):
    import yaml
    from tc_light_amd.dataparser import write_mjpeg_avi
    from tc_light_amd.evaluate import read_video_u8, warp_ssim
    from tc_light_amd.raft import RAFTEngine, seeded_state_dict
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (1, 150, 220, 3), dtype=np.uint8)
    src = np.stack([np.roll(base[0], (k, 2 * k), (0, 1)) for k in range(4)])            # 4 frames, 150 x 220 (resized to the edit size)
    edit = np.clip(src[:, 5:135, 7:205].astype(np.int32) + 20, 0, 255).astype(np.uint8)  # 130 x 198: padded to 136 x 200 for RAFT
    write_mjpeg_avi(str(tmp_path / "output.avi"), edit)
    write_mjpeg_avi(str(tmp_path / "output_gt.avi"), src)
    cfg = {"generation": {"prompt": {"a": "soft light", "b": "warm light"}}, "models": {"raft": str(tmp_path / "absent.pth")},
           "sec_per_frame": 0.5, "max_memory_allocated": 1000.0, "total_number_of_frames": 4, "total_time": 2.0}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, TCL_ALLOW_RANDOM_WEIGHTS="1")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "evaluate.py"), "--output_dir", str(tmp_path), "--eval_cost"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "clip-frame" in r.stdout and "pick-score" in r.stdout
    lines = (tmp_path / "result.txt").read_text().splitlines()
    assert lines[0] == "unknown_video - warm light"                                      # the last prompt's block
    keys = [ln.split(": ")[0] for ln in lines[1:]]
    assert keys == ["warp-error-ssim", "z_fps", "z_max_memory_allocated(M)", "z_resolution", "z_total_frames", "z_total_time(s)"]
    vals = dict(ln.split(": ") for ln in lines[1:])
    assert vals["z_fps"] == "2.0000" and vals["z_total_frames"] == "4.0000" and vals["z_resolution"] == f"{np.sqrt(130 * 198):.4f}"
    e, s = read_video_u8(str(tmp_path / "output.avi")), read_video_u8(str(tmp_path / "output_gt.avi"))
    score, _ = warp_ssim(e, s, RAFTEngine(seeded_state_dict(), dev))
    assert vals["warp-error-ssim"] == f"{score * 100:.2f}"
