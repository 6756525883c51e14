"""CPU: bench.py's host side -- its threaded input synthesis gives tests/synth.py::video_clip's arrays bit for bit, --dump-outputs writes what
it says, and --steps / --warmup are checked before anything runs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,h,w,seed", [(1, 8, 8, 12345), (5, 24, 40, 12345), (12, 33, 17, 7)])
def test_video_clip_bit_identical_to_synth(n, h, w, seed):
    fast = bench.video_clip(n, h, w, seed=seed)
    ref = synth.video_clip(n, h, w, seed=seed)
    for k in ("frames", "past_flows", "masks"):
        a, b = fast[k].numpy(), ref[k].numpy()
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


def test_dump_outputs(tmp_path):
    g = torch.Generator().manual_seed(0)
    out = torch.rand(7, 3, 16, 24, generator=g)
    info = dict(losses_exposure=torch.rand(5, generator=g), losses_unique=torch.rand(9, generator=g))
    bench.dump_outputs(str(tmp_path), out, info, frames_bytes=2 * 3 * 16 * 24 * 4, sample=100)
    f = np.load(tmp_path / "relit_frames.npy")
    assert f.dtype == np.float32 and np.array_equal(f, out[[0, 3]].numpy())          # frames 0 and N/2: two fit the budget
    s, i = np.load(tmp_path / "relit_sample.npy"), np.load(tmp_path / "relit_sample_index.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and 0 < len(s) == len(i) <= 100
    assert np.array_equal(s, out.reshape(-1).numpy()[i.astype(np.int64)])
    for k in ("losses_exposure", "losses_unique"):
        v = np.load(tmp_path / (k + ".npy"))
        assert v.dtype == np.float64 and np.array_equal(v, info[k].double().numpy())
    again = tmp_path / "again"
    bench.dump_outputs(str(again), out, info, frames_bytes=2 * 3 * 16 * 24 * 4, sample=100)
    assert np.array_equal(np.load(again / "relit_sample_index.npy"), i)                 # the sample is fixed


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_bad_step_counts(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps must be >= 1" in p.stderr
