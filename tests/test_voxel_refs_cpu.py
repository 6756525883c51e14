"""CPU: the references of tests/voxel_refs.py against the reference's own voxelization (tests/golden/voxel.npz, written by
tests/golden/make_golden_voxel.py), so that the GPU tests compare against yardsticks that are themselves pinned."""
import numpy as np
import pytest
import torch

import voxel_refs as R


@pytest.mark.parametrize("case,use_voxel,use_inst", [("vox", True, False), ("vox_inst", True, True), ("inst_only", False, True)])
def test_voxelization_ref_matches_reference(golden, case, use_voxel, use_inst):
    g = golden("voxel")
    ids, rgb, xyz = (torch.from_numpy(g[k]) for k in ("flow_ids", "rgb", "xyz"))
    inst = torch.from_numpy(g["instance"]) if use_inst else None
    inv = R.voxelization_ref(ids.reshape(-1), R.rows_nchw(rgb), R.rows_nchw(xyz), float(g["voxel_size"]) if use_voxel else None, inst)
    want = g[case + "_inv"]
    assert int(inv.max()) + 1 == int(want.max()) + 1
    assert np.array_equal(R.canon(inv), R.canon(want))
    if use_voxel:                                        # merging is really exercised by the fixture
        assert int(want.max()) + 1 < 0.9 * (int(ids.max()) + 1)


def test_canon_is_first_appearance():
    assert R.canon(np.array([7, 7, 2, 9, 2, 7])).tolist() == [0, 0, 1, 2, 1, 0]
    assert R.canon(torch.tensor([3, 1, 1, 3])).tolist() == R.canon(torch.tensor([0, 5, 5, 0])).tolist()


def test_floor_div_ref_spot():
    a = torch.tensor([0.0, 1.0, -1.0, 2.5, -2.5, 7.0, -7.0, 0.3, -0.0], dtype=torch.float32)
    assert R.floor_div_ref(a, 2.0).tolist() == [0.0, 0.0, -1.0, 1.0, -2.0, 3.0, -4.0, 0.0, -0.0]
    x = torch.tensor([1.25, np.nextafter(np.float32(1.25), np.float32(0)), 1.125, -1.25, np.nextafter(np.float32(-1.25), np.float32(-2))],
                     dtype=torch.float32)
    assert R.floor_div_ref(x, 0.25).tolist() == [5.0, 4.0, 4.0, -5.0, -6.0]   # exact multiples and one ulp either side
    assert torch.signbit(R.floor_div_ref(torch.tensor([-0.0]), 2.0)).item()


def test_track_mean_ref_order_and_division():
    vals = torch.tensor([[[[1e8, 1.0]]], [[[1.0, 3.0]]], [[[-1e8, 5.0]]]], dtype=torch.float32)      # N=3, C=1, 1x2
    ids = torch.tensor([[[0, 1]], [[0, 1]], [[0, 2]]], dtype=torch.int32)
    mean, cnt = R.track_mean_ref(vals, ids, 4)
    assert cnt.tolist() == [3.0, 2.0, 1.0, 0.0]
    assert mean[:, 0].tolist() == [0.0, 2.0, 5.0, 0.0]   # (1e8 + 1) - 1e8 in f32, frame order: 0; an empty track: 0 / max(0, 1)
