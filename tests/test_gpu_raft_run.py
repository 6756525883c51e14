"""GPU: run.py with data.flow_model: raft on the tiny clip of test_gpu_run.py (4 frames, 192x256, seeded weights, 1 step): the flow cache holds
RAFT flows in <video>_{future,past}_flow_raft/ (not MemFlowNet's), no memflow directory appears, and the cached tensors are what
estimate_flows_raft computes from the same frames and weights."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_run_py_with_raft_flows(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.join(os.path.dirname(__file__), "..")
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(__file__))
    import synth
    import run
    from tc_light_amd.dataparser import VideoDataParser
    from tc_light_amd.model_utils import load_raft_state
    from tc_light_amd.raft import RAFTEngine, estimate_flows_raft
    d = synth.video_clip(4, 192, 256, seed=2)
    vid = tmp_path / "clip.npy"
    np.save(vid, (d["frames"].permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{rgb_path: {vid}, height: 192, width: 256, flow_model: raft}}
generation:
  prompt: {{edit: "warm light"}}
  n_timesteps: 1
  alpha_t: 0.01
  frame_range: [0, 4, 1]
post_opt: {{epochs_exposure: 1, epochs: 1, batch_size: 4}}
models: {{allow_random: true, raft: {tmp_path / 'absent' / 'raft-things.pth'}}}
""")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        run.main(["--config", str(cfg)])
    finally:
        os.chdir(cwd)
    assert not any("flow_memflow" in f for f in os.listdir(tmp_path))
    cached = {}
    for kind in ("future", "past"):
        dd = tmp_path / f"clip_{kind}_flow_raft"
        files = sorted(os.listdir(dd))
        assert files == [f"{i:04d}.pt" for i in range(4)]
        cached[kind] = torch.cat([torch.load(dd / f) for f in files])
        assert tuple(torch.load(dd / files[1]).shape) == (1, 2, 192, 256)
    parser = VideoDataParser({"rgb_path": str(vid), "height": 192, "width": 256, "flow_model": "raft"}, "cuda")
    frames = parser.load_video(list(range(4)))
    with pytest.warns(UserWarning):
        eng = RAFTEngine(load_raft_state(None, allow=True), "cuda")
    fut, past = estimate_flows_raft(eng, frames)
    assert torch.equal(cached["future"], fut.cpu()) and torch.equal(cached["past"], past.cpu())
    assert cached["future"][3].abs().max().item() == 0 and cached["past"][0].abs().max().item() == 0
