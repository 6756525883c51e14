"""CPU: the host side of the SceneFlow parser (tc_light_amd/sceneflow.py) -- PFM and camera-file readers, path layout, validation -- and the
data.scene_type dispatch of run.py, reached without a device."""
import os

import numpy as np
import pytest

from sceneflow_files import cam_text as _cam_text, write_pfm
from tc_light_amd import sceneflow as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("little", [True, False])
@pytest.mark.parametrize("ch", [1, 3])
def test_pfm_round_trip(tmp_path, little, ch):
    g = np.random.default_rng(ch + 2 * little)
    a = g.standard_normal((5, 7, 3) if ch == 3 else (5, 7)).astype(np.float32)
    a[0, 0] = 123.5                                      # top-left stays top-left: rows are flipped back
    p = tmp_path / "x.pfm"
    write_pfm(p, a, little=little, scale=2.0)
    b, scale = S.read_pfm(str(p))
    assert b.dtype == np.float32 and b.shape == a.shape and scale == 2.0
    assert np.array_equal(a, b)


def test_pfm_rejects_other_files(tmp_path):
    p = tmp_path / "bad.pfm"
    p.write_bytes(b"P6\n2 2\n255\n" + bytes(12))
    with pytest.raises(ValueError):
        S.read_pfm(str(p))
    write_pfm(p, np.zeros((4, 4), np.float32))
    p.write_bytes(p.read_bytes()[:-8])
    with pytest.raises(ValueError):
        S.read_pfm(str(p))


def test_camera_file(tmp_path):
    g = np.random.default_rng(0)
    frames = [(6 + i, g.standard_normal((4, 4)), g.standard_normal((4, 4))) for i in range(3)]
    p = tmp_path / "camera_data.txt"
    p.write_text(_cam_text(frames))
    cams = S.read_camera_data(str(p))
    assert [c["frame_id"] for c in cams] == [6, 7, 8]
    for c, (_, L, R) in zip(cams, frames):
        assert np.array_equal(c["left"], L) and np.array_equal(c["right"], R)
    p.write_text("Frame 1\nL 1 2 3\nR 1 2 3\n\n")
    with pytest.raises(ValueError):
        S.read_camera_data(str(p))


def test_paths_defaults_and_validation(tmp_path):
    sp = "35mm_focallength/scene_forwards/slow"
    cam = tmp_path / "camera_data" / sp
    cam.mkdir(parents=True)
    (cam / "camera_data.txt").write_text(_cam_text([(1, np.eye(4), np.eye(4)), (2, np.eye(4), np.eye(4))]))
    p = S.SceneFlowDataParser({"data_dir": str(tmp_path), "scene_path": sp, "stereo_sel": "right", "height": 64, "width": 96}, "cpu")
    j = os.path.join
    assert p.rgb_path == j(str(tmp_path), "frames_cleanpass", sp, "right")
    assert p.disparity_path == j(str(tmp_path), "disparity", sp, "right")
    assert p.future_flow_path == j(str(tmp_path), "optical_flow", sp, "into_future", "right")
    assert p.past_flow_path == j(str(tmp_path), "optical_flow", sp, "into_past", "right")
    assert p.intrinsics == (1050.0, 1050.0, 479.5, 269.5) and p.n_frames == 2
    assert (p.alpha, p.fps, p.voxel_size, p.contract, p.use_raft) == (0.1, 30, None, False, False)
    d = S.SceneFlowDataParser({"height": 8, "width": 8}, "cpu")
    assert (d.data_dir, d.scene_path, d.stereo_sel) == ("data/sceneflow", "15mm_focallength/scene_backwards/fast", "left")
    assert d.intrinsics == (450.0, 450.0, 479.5, 269.5)
    for bad in ({"stereo_sel": "middle"}, {"scene_path": "20mm_focallength/scene_forwards/slow"}, {"scene_path": "15mm_focallength/scene_up/slow"},
                {"scene_path": "15mm_focallength/scene_forwards/medium"}, {"scene_path": "15mm_focallength"}):
        with pytest.raises(ValueError):
            S.SceneFlowDataParser({"height": 8, "width": 8, **bad}, "cpu")


def test_example_config_loads():
    from tc_light_amd.config_utils import load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_sceneflow.yaml")], print_config=False)
    finally:
        os.chdir(cwd)
    assert c.data.scene_type == "sceneflow" and c.data.voxel_size is not None and c.post_opt.apply_opt


@pytest.mark.parametrize("scene_type,word", [("carla", "not yet built"), ("interiornet", "not yet built"), ("bogus", "not supported")])
def test_run_scene_type_dispatch_raises_before_models(tmp_path, monkeypatch, scene_type, word):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before data.scene_type was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{scene_type: {scene_type}, height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}}}
""")
    with pytest.raises(NotImplementedError, match=word) as e:
        run.main(["--config", str(cfg)])
    if word == "not yet built":
        assert scene_type in str(e.value)
