"""CPU: RAFT's host surface -- the parameter map against the reference's state dict (tests/golden/raft.npz), the checkpoint loader, the flow-model
dispatch and the size checks.  No GPU."""
import os

import numpy as np
import pytest
import torch


def test_param_shapes_match_reference(golden):
    from tc_light_amd.raft import raft_param_shapes
    G = golden("raft")
    ref = {}
    for item in str(G["keys"]).split(";"):
        k, s = item.split(":")
        ref[k] = tuple(int(x) for x in s.split(",") if x)
    assert raft_param_shapes() == ref


def test_seeded_state_dict_covers_every_key():
    from tc_light_amd.raft import raft_param_shapes, seeded_state_dict
    sd, sh = seeded_state_dict(), raft_param_shapes()
    assert set(sd) == set(sh) and all(tuple(sd[k].shape) == s for k, s in sh.items())


def test_load_raft_state_strips_module_prefix(tmp_path):
    from tc_light_amd.model_utils import load_raft_state
    sd = {"module.fnet.conv1.weight": torch.ones(64, 3, 7, 7), "module.update_block.mask.2.bias": torch.arange(576.)}
    p = tmp_path / "raft-things.pth"
    torch.save(sd, p)
    got = load_raft_state(str(p))
    assert set(got) == {"fnet.conv1.weight", "update_block.mask.2.bias"}
    assert torch.equal(got["update_block.mask.2.bias"], torch.arange(576.))


def test_load_raft_state_missing_file(tmp_path):
    from tc_light_amd.model_utils import load_raft_state
    from tc_light_amd.raft import raft_param_shapes
    with pytest.raises(FileNotFoundError):
        load_raft_state(str(tmp_path / "absent.pth"))
    with pytest.warns(UserWarning):
        sd = load_raft_state(str(tmp_path / "absent.pth"), allow=True)
    assert set(sd) == set(raft_param_shapes())


def test_unknown_flow_model_is_an_error(tmp_path):
    from tc_light_amd.dataparser import VideoDataParser
    for name, ok in (("memflow", True), ("RAFT", True), ("raft", True), ("flownet2", False), (None, False)):
        p = VideoDataParser({"rgb_path": str(tmp_path / "clip.npy"), "height": 128, "width": 192, "flow_model": name}, "cpu")
        if ok:
            assert p.flow_model_name() in ("memflow", "raft")
            continue
        with pytest.raises(ValueError, match="memflow.*raft"):
            p.flow_model_name()
        with pytest.raises(ValueError):
            p.make_flow_engine({"allow_random": True}, True)
        with pytest.raises(ValueError):
            p.estimate_and_cache_flow(torch.zeros(2, 3, 128, 192), [0, 1], None, save_flow=False)


def test_size_checks():
    from tc_light_amd.raft import check_size
    check_size(128, 192)
    check_size(720, 1280)
    for H, W in ((130, 192), (128, 196), (64, 96), (128, 120), (120, 192)):
        with pytest.raises(ValueError):
            check_size(H, W)


def test_useful_flop_count():
    from tc_light_amd.raft import useful_flops
    f = useful_flops(720, 1280)
    P = 90 * 160
    assert abs(f["update"] / 20 - 63.0e9) < 1.0e9                      # ~77 GFLOP per iteration without the context fold, ~63 with it
    assert f["fold"] == 2 * P * 2 * 5 * 128 * 384
    assert 0.09e12 < f["encoders"] / 3 < 0.15e12
