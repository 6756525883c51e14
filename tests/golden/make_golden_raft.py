"""Golden vectors for RAFT (data.flow_model: raft): the REFERENCE RAFT (utils/evaluation/core/raft.py) and VideoDataParser.load_flow, loaded with
the seeded stand-in weights of tc_light_amd.raft (strict=True) and run on the CPU.  Run from the repo root:
python tests/golden/make_golden_raft.py  (needs /root/reference; writes raft.npz; the weights are regenerated from the seed by the tests)."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
REF = "/root/reference"
sys.path.insert(0, ROOT)
from tc_light_amd import raft as TR  # noqa: E402  (shapes / seeded weights only; the library loads lazily, none is needed here)

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "utils", "evaluation"))


class _Stub(types.ModuleType):
    """Stands in for optional packages the RAFT path never calls (video I/O, metrics, model zoos) but whose modules import them."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(f"{self.__name__}.{name}")

    def __call__(self, *a, **k):
        return self


def import_with_stubs(modname):
    import importlib
    for _ in range(50):
        try:
            return importlib.import_module(modname)
        except ModuleNotFoundError as e:
            if e.name is None or e.name.split(".")[0] in ("utils", "core"):
                raise
            sys.modules[e.name] = _Stub(e.name)
    raise RuntimeError(f"could not import {modname}")


RAFT = import_with_stubs("core.raft").RAFT

torch.manual_seed(0)
torch.set_num_threads(min(16, os.cpu_count() or 8))
SEED = 5
model = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).eval()
ref_sd = model.state_dict()
shapes = TR.raft_param_shapes()
assert set(shapes) == set(ref_sd) and all(tuple(ref_sd[k].shape) == tuple(s) for k, s in shapes.items())
model.load_state_dict(TR.seeded_state_dict(SEED), strict=True)

out = {"seed": SEED, "keys": np.array(";".join(f"{k}:{','.join(map(str, v.shape))}" for k, v in ref_sd.items()))}
g = np.random.default_rng(17)


def smooth_clip(n, H, W, rng):
    """n frames in [0, 1]: a smooth random texture translated by a few pixels per frame (a flow worth estimating)."""
    base = torch.from_numpy(rng.random((1, 3, H // 8 + 4, W // 8 + 4)).astype(np.float32))
    big = torch.nn.functional.interpolate(base, size=(H + 32, W + 32), mode="bicubic", align_corners=False).clamp(0, 1)
    u8 = (torch.cat([big[:, :, 2 * i:2 * i + H, 3 * i:3 * i + W] for i in range(n)]) * 255).round().to(torch.uint8)
    return u8, u8.float() / 255.0                                  # stored as uint8; the tests rebuild the f32 frames as u8 / 255


with torch.no_grad():
    u8, img = smooth_clip(1, 64, 96, g)
    out["enc_img_u8"] = u8.numpy()
    for conv, scale in (("01", 1.0), ("255", 255.0)):
        x = 2 * (img * scale / 255.0) - 1.0
        out[f"fnet_{conv}"] = model.fnet(x).numpy()
        out[f"cnet_{conv}"] = model.cnet(x).numpy()
    u8, clip4 = smooth_clip(4, 128, 192, g)
    out["clip_u8"] = u8.numpy()                                      # the load_flow clip; its first two frames are the 128x192 pair
    for H, W in ((128, 192), (144, 256)):
        if H == 128:
            clip = clip4[:2]
        else:
            u8, clip = smooth_clip(2, H, W, g)
            out[f"pair_{H}x{W}_u8"] = u8.numpy()                    # [2,3,H,W]: image1, image2
        for conv, scale in (("01", 1.0), ("255", 255.0)):
            low, up = model(clip[0:1] * scale, clip[1:2] * scale, iters=20, test_mode=True)
            out[f"low_{H}x{W}_{conv}"] = low.numpy()
            out[f"up_{H}x{W}_{conv}"] = up[..., ::2, ::2].numpy()      # every other pixel in each direction (fixture size)

# ---- VideoDataParser.load_flow, raft branch, with prepare_raft_model returning the seeded model
import importlib.util  # noqa: E402

sys.modules["utils.VidToMe"] = _Stub("utils.VidToMe")              # the frame loader (frames are passed in as gts) and its diffusers / ControlNet imports
_spec = importlib.util.spec_from_file_location("video_dataparser", os.path.join(REF, "utils", "dataparsers", "video_dataparser.py"))
V = importlib.util.module_from_spec(_spec)
for _ in range(50):
    try:
        _spec.loader.exec_module(V)
        break
    except ModuleNotFoundError as e:
        if e.name is None or e.name.split(".")[0] in ("utils", "core"):
            raise
        sys.modules[e.name] = _Stub(e.name)
import tempfile  # noqa: E402

clip = clip4
with tempfile.TemporaryDirectory() as td:
    rgb = os.path.join(td, "frames")
    os.makedirs(rgb)
    open(os.path.join(rgb, "0000.png"), "w").close()
    cfg = types.SimpleNamespace(rgb_path=rgb, height=128, width=192, flow_model="raft")
    V.eu.prepare_raft_model = lambda device: model
    dp = V.VideoDataParser(cfg, device="cpu")
    dp.process_flow = lambda fl: torch.stack(fl)                  # the flows are at the working size already (its resize is the identity)
    dp.load_flow(list(range(4)), future_flow=True, past_flow=False, gts=clip.clone())
    fut = [torch.load(os.path.join(rgb, "future_flow_raft", f"{i:04d}.pt")) for i in range(4)]
    dp.load_flow(list(range(4)), future_flow=False, past_flow=True, gts=clip.clone())
    past = [torch.load(os.path.join(rgb, "past_flow_raft", f"{i:04d}.pt")) for i in range(4)]
out["load_flow_future"] = torch.cat(fut)[..., ::2, ::2].numpy()
out["load_flow_past"] = torch.cat(past)[..., ::2, ::2].numpy()

# outputs in f16 (their rounding, ~5e-4 relative, is far below the tests' tolerances): the fixture stays under 1 MiB
out = {k: (v.astype(np.float16) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in out.items()}
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "raft.npz"), **out)
print({k: (v.shape, float(np.abs(v).mean())) for k, v in out.items() if hasattr(v, "shape") and v.ndim > 0 and v.dtype.kind == "f"})
print(os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "raft.npz")), "bytes")
