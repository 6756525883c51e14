"""CPU: the host surface the two flow estimators share (tc_light_amd.flow_core, hostlogic.memflow_splitkv_chunks, hostlogic.pad8_amounts):
the chunk chooser against values worked out by hand, the weight packing against explicit loops, the one padding rule, and that the three flow
modules import without the shared library.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tc_light_amd.hostlogic import memflow_splitkv_chunks, pad8_amounts


# a chunk count c fits when T % (64 c) == 0 and ceil(P / 128) * c <= 1024; the expected values below are worked out from that rule by hand
@pytest.mark.parametrize("P,T,want,expected", [
    (14400, 14400, 3, 3),        # 1280x720: 14400 = 75 * 192; 113 * 3 = 339 blocks
    (14400, 28800, 3, 3),        # a working memory of two frames: 28800 = 150 * 192
    (384, 384, 3, 3),            # 128x192: 384 = 2 * 192
    (384, 768, 3, 3),            # 768 = 4 * 192
    (320, 320, 3, 5),            # 320 = 64 * 5, not a multiple of 192 or 128 (nor 256, 384): 5 is the first of (3, 2, 5, 4, 6) that fits
    (2240, 2240, 3, 5),          # 2240 = 7 * 320 = 11 * 192 + 128 = 17 * 128 + 64
    (425, 425, 3, 0),            # 136x200: 425 is odd
    (425, 850, 3, 0),            # 850 = 13 * 64 + 18
    (43777, 384, 3, 2),          # ceil(43777 / 128) = 343 blocks of queries: 343 * 3 = 1029 > 1024, 343 * 2 = 686; 384 = 3 * 128
    (43777, 192, 3, 0),          # ... and 192 is no multiple of 128, 320, 256 or 384: 3 is barred by the blocks, nothing else divides
    (131072, 384, 3, 0),         # 1024 blocks of queries: no chunk count >= 2 fits the grid
    (14400, 14400, 0, 0),        # a want below 2 asks for the one-pass kernel
    (14400, 14400, 1, 0),
    (14400, 14400, 2, 3),        # 14400 = 112 * 128 + 64: the wanted 2 does not fit, 3 is the first of the list that does
    (384, 768, 2, 2),            # 768 = 6 * 128: the wanted count fits and is kept
    (384, 768, 4, 4),            # 768 = 3 * 256
    (384, 768, 5, 3),            # 768 = 2 * 320 + 128: 5 does not fit -> the list from its start
    (384, 1920, 5, 5),           # 1920 = 6 * 320
    (384, 768, 6, 6),            # 768 = 2 * 384
])
def test_memflow_splitkv_chunks_against_hand_values(P, T, want, expected):
    assert memflow_splitkv_chunks(P, T, want) == expected
    if want == 3:
        assert memflow_splitkv_chunks(P, T) == expected                                 # the default


def test_conv3_weights_on_a_tiny_tensor():
    from tc_light_amd.flow_core import conv3_weights
    co, ci, co_pad, ci_pad = 3, 2, 64, 64
    g = torch.Generator().manual_seed(2)
    w = torch.randn(co, ci, 3, 3, generator=g).half().float()                           # f16-representable: the packing must not change a value
    b = torch.randn(co, generator=g).half().float()
    pw, pb, pci, pco = conv3_weights(w, b, co_pad, ci_pad)
    assert (pci, pco) == (ci_pad, co_pad) and pw.dtype == pb.dtype == torch.float16 and pw.is_contiguous() and pb.is_contiguous()
    assert tuple(pw.shape) == (co_pad, 9 * ci_pad) and tuple(pb.shape) == (co_pad,)
    want = torch.zeros(co_pad, 9 * ci_pad)
    for o in range(co):
        for c in range(ci):
            for ky in range(3):
                for kx in range(3):
                    want[o, (ky * 3 + kx) * ci_pad + c] = w[o, c, ky, kx]
    assert torch.equal(pw.float(), want)                                                # padding rows and columns are zero: `want` started as zeros
    assert torch.equal(pb[:co].float(), b) and not pb[co:].any()
    assert int((pw != 0).sum()) == int((w != 0).sum())
    # input channels left as they are (RAFT's update block: only the outputs are padded)
    qw, qb, qci, qco = conv3_weights(w, b, 64)
    assert (qci, qco) == (ci, 64) and tuple(qw.shape) == (64, 9 * ci)
    for o in range(co):
        for c in range(ci):
            for t in range(9):
                assert qw[o, t * ci + c].item() == w[o, c, t // 3, t % 3].item()
    assert not qw[co:].any() and not qb[co:].any()


def test_lin_padding():
    from tc_light_amd.flow_core import Lin, pad_to, up64
    assert [up64(c) for c in (1, 64, 65, 126, 324)] == [64, 64, 128, 128, 384]
    w = torch.arange(1.0, 7.0).view(3, 2, 1, 1)
    b = torch.tensor([0.5, -1.0, 2.0])
    lin = Lin(w, b, "cpu")
    assert (lin.ci, lin.co) == (64, 64) and tuple(lin.w.shape) == (64, 64) and tuple(lin.b.shape) == (64,)
    assert lin.w.dtype == lin.b.dtype == torch.float16 and lin.w.is_contiguous()
    want = torch.zeros(64, 64)
    for o in range(3):
        for c in range(2):
            want[o, c] = w[o, c, 0, 0]
    assert torch.equal(lin.w.float(), want)
    assert torch.equal(lin.b[:3].float(), b) and not lin.b[3:].any()
    nob = Lin(w, None, "cpu")
    assert tuple(nob.b.shape) == (64,) and nob.b.dtype == torch.float16 and not nob.b.any() and torch.equal(nob.w, lin.w)
    t = torch.ones(2, 3)
    assert pad_to(t, 1, 3) is t and torch.equal(pad_to(t, 0, 4), torch.cat([t, torch.zeros(2, 3)]))


@pytest.mark.parametrize("H", [120, 121, 127, 128])
@pytest.mark.parametrize("W", [120, 121, 127, 128])
def test_pad8_amounts_is_the_input_padder_formula(H, W):
    # eval_utils.InputPadder.__init__: pad_ht = (((ht // 8) + 1) * 8 - ht) % 8, likewise pad_wd; _pad = [wd // 2, wd - wd // 2, ht // 2, ht - ht // 2]
    pad_ht = (((H // 8) + 1) * 8 - H) % 8
    pad_wd = (((W // 8) + 1) * 8 - W) % 8
    assert pad8_amounts(H, W) == (pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2)
    l, r, t, b = pad8_amounts(H, W)
    assert (H + t + b) % 8 == 0 and (W + l + r) % 8 == 0 and t + b < 8 and l + r < 8 and 0 <= b - t <= 1 and 0 <= r - l <= 1


def test_the_two_padders_pad_a_ramp_to_the_same_pixels():
    from tc_light_amd.flow_core import pad8
    from tc_light_amd.lpips import pad8_u8
    ramp = torch.arange(45, dtype=torch.uint8).view(1, 5, 9, 1).repeat(1, 1, 1, 3)      # [N,H,W,3] uint8, every pixel its own value
    a = pad8_u8(ramp)
    b, pad = pad8(ramp.permute(0, 3, 1, 2).float())
    assert pad == list(pad8_amounts(5, 9)) == [3, 4, 1, 2]
    assert tuple(a.shape) == (1, 8, 16, 3) and torch.equal(a.permute(0, 3, 1, 2).float(), b)
    assert torch.equal(a[0, 1:6, 3:12], ramp[0]) and a[0, 0, 0, 0] == 0 and a[0, -1, -1, 0] == 44   # the ramp in place, corners replicated


def test_flow_modules_import_without_the_library():
    code = ("import sys\n"
            "import tc_light_amd.flow_core, tc_light_amd.memflow, tc_light_amd.raft\n"
            "import tc_light_amd.lib as L\n"
            "assert L._lib is None, 'the shared library was loaded on import'\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n"
            "from tc_light_amd import memflow as MF, raft as RF\n"
            "assert len(MF.memflow_param_shapes()) > 100 and len(RF.raft_param_shapes()) > 100\n"
            "assert L._lib is None\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TCL_LIB_PATH=os.path.join(root, "no_such_dir", "libtclight_hip.so"))       # a path that does not exist: loading it would raise
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_memflow_keeps_the_names_its_callers_use():
    from tc_light_amd import flow_core as FC, memflow as MF
    assert MF.seeded_state_dict is FC.seeded_state_dict and MF.CorrBlock is FC.CorrBlock and MF.EncoderEngine is FC.EncoderEngine
    sd = MF.seeded_state_dict(MF.encoder_param_shapes("", "batch"), 3)
    assert set(sd) == set(FC.encoder_param_shapes("", "batch")) and np.isfinite(sd["conv1.weight"].numpy()).all()
    import inspect
    assert list(inspect.signature(MF.estimate_flows).parameters) == ["engine", "frames", "warm_start"]
    assert inspect.signature(MF.MemFlowEngine.__init__).parameters["splitkv"].default == 3
    assert inspect.signature(FC.CorrBlock.lookup_rows).parameters["tiled"].default is True
