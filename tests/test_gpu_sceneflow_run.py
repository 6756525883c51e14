"""GPU: run.py end to end on a synthetic SceneFlow tree (data.scene_type: sceneflow): PNG frames, disparity and flow PFMs and camera_data.txt of
a slowly translating fronto-parallel textured plane -> device unprojection, ground-truth flows, masks, track ids, voxelised Unique Video Tensor ->
relighting (1 denoising step) -> stage 1/2 -> output.npy + config.yaml.  Seeded random weights: plumbing and formats, not image quality."""
import os

import numpy as np
import pytest
import torch
import yaml

import synth
import voxel_refs as R
from sceneflow_files import cam_text as _cam_text, write_pfm

pytestmark = pytest.mark.gpu

SCENE = "15mm_focallength/scene_backwards/fast"
N, H, W, SX, SY, DEPTH, FX, FIRST = 4, 192, 256, 2, 1, 4.5, 450.0, 6


def write_tree(root):
    """frame k (u) = base(u + k s): the camera moves by k s pixels = k s DEPTH / FX world units; pixel pitch in the world 0.01."""
    from PIL import Image
    fr = (torch.floor(synth.video_clip(N, H, W, seed=9, shift=(SX, SY), jitter=0.0)["frames"] * 4) / 4 + 0.1).clamp(0, 1)
    u8 = (fr.permute(0, 2, 3, 1).numpy() * 255).round().astype(np.uint8)
    d = {k: os.path.join(root, *p) for k, p in dict(rgb=("frames_cleanpass", SCENE, "left"), disp=("disparity", SCENE, "left"),
                                                    fut=("optical_flow", SCENE, "into_future", "left"),
                                                    past=("optical_flow", SCENE, "into_past", "left"), cam=("camera_data", SCENE)).items()}
    for p in d.values():
        os.makedirs(p)
    cams = []
    for k in range(N):
        fid = FIRST + k
        Image.fromarray(u8[k]).save(os.path.join(d["rgb"], f"{fid:04d}.png"))
        write_pfm(os.path.join(d["disp"], f"{fid:04d}.pfm"), np.full((H, W), FX / DEPTH, np.float32), little=(k % 2 == 0))
        fut = np.zeros((H, W, 3), np.float32); past = np.zeros((H, W, 3), np.float32)
        if k < N - 1:
            fut[..., 0], fut[..., 1] = -SX, -SY
        if k > 0:
            past[..., 0], past[..., 1] = SX, SY
        fut[..., 2] = past[..., 2] = 7.0                 # the third channel is not flow and must be ignored
        write_pfm(os.path.join(d["fut"], f"OpticalFlowIntoFuture_{fid:04d}_L.pfm"), fut)
        write_pfm(os.path.join(d["past"], f"OpticalFlowIntoPast_{fid:04d}_L.pfm"), past, little=False)
        m = np.eye(4)
        m[0, 3], m[1, 3] = k * SX * DEPTH / FX, -k * SY * DEPTH / FX
        cams.append((fid, m, m + np.diag([0, 0, 0, 0])))
    with open(os.path.join(d["cam"], "camera_data.txt"), "w") as f:
        f.write(_cam_text(cams))


def test_run_py_sceneflow(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.join(os.path.dirname(__file__), "..")
    import run
    from tc_light_amd.sceneflow import SceneFlowDataParser
    tree = tmp_path / "sceneflow"
    write_tree(str(tree))
    data = dict(scene_type="sceneflow", data_dir=str(tree), scene_path=SCENE, stereo_sel="left", voxel_size=0.03, height=H, width=W)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump(dict(
        base_config=os.path.join(root, "configs", "tclight_default.yaml"), work_dir=str(tmp_path / "work"), data=data,
        generation=dict(prompt=dict(edit="warm light"), n_timesteps=1, alpha_t=0.01, frame_range=[0, N, 1]),
        post_opt=dict(epochs_exposure=1, epochs=1, batch_size=4), models=dict(allow_random=True))))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        run.main(["--config", str(cfg)])
    finally:
        os.chdir(cwd)
    outs = [os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "work") for f in fs if f == "output.npy"]
    assert len(outs) == 1
    out = np.load(outs[0])
    assert out.shape == (N, H, W, 3) and np.isfinite(out.astype(np.float64)).all()
    saved = yaml.safe_load(open(os.path.join(os.path.dirname(outs[0]), "config.yaml")))
    assert saved["sec_per_frame"] > 0 and saved["data"]["scene_type"] == "sceneflow"

    dev = torch.device("cuda:0")
    s = SceneFlowDataParser(data, dev).load_data(list(range(N)))
    assert tuple(s["frames"].shape) == (N, 3, H, W) and tuple(s["p_world"].shape) == (N, 3, H, W)
    assert s["flows"][:, :2].abs().max().item() == SX and s["flows"][-1].abs().max().item() == 0 and s["past_flows"][0].abs().max().item() == 0
    want = R.voxelization_ref(s["flow_ids"].cpu().reshape(-1), R.rows_nchw(s["frames"].cpu()), R.rows_nchw(s["p_world"].cpu()), 0.03)
    assert np.array_equal(R.canon(s["inv"]), R.canon(want))
    assert s["k"] == int(want.max()) + 1
    assert s["n_tracks"] < N * H * W                     # tracks persist
    assert s["k"] < s["n_tracks"]                        # and voxels merge tracks
    plain = SceneFlowDataParser(dict(data, voxel_size=None), dev).load_data(list(range(N)))
    assert torch.equal(plain["inv"], plain["flow_ids"].reshape(-1)) and plain["k"] == plain["n_tracks"]
