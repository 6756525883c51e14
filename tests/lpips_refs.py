"""A float64 torch restatement of the frame-lpips figure (utils/evaluation/eval_utils.py:368-386 FrameLPIPS on lpips.LPIPS(net='vgg'), LPIPS v0.1),
the reference the tests of tc_light_amd/lpips.py are held to.  Two modes:
  exact: everything in float64;
  f16 floor (f16=True): the output of the stem, of every convolution (after bias and ReLU) and of every pool is rounded to f16, the head stays in
    float64.  This is what an f16 engine with exact arithmetic between its roundings would give: the project's usual floor.
`s` is the engine's input scale: the scaled image and every bias are multiplied by s and the head's eps too, which leaves the exact result unchanged
for a power of two (tests/test_lpips_refs_cpu.py proves it) and places the f16 roundings where the engine has them.
The stand-in weights are tc_light_amd.lpips.seeded_state: tests and engine draw the same tensors."""
import numpy as np
import torch
import torch.nn.functional as F

from tc_light_amd.lpips import CHANNELS, EPS, GROUPS, SCALE, SHIFT, seeded_state  # noqa: F401  (seeded_state: re-exported for the tests)

F64 = torch.float64


def _r16(t):
    return t.to(torch.float16).to(F64)


def scaling_layer(x, s=1.0):
    """x [N,3,H,W] float64 in 0..255 -> (x - shift) / scale * s."""
    shift = torch.tensor(SHIFT, dtype=F64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=F64).view(1, 3, 1, 1)
    return (x - shift) / scale * s


def taps(x, state, s=1.0, f16=False, n_taps=5):
    """x [N,3,H,W] float64 in 0..255 -> the first n_taps of the five tapped feature maps [N,C,h,w] float64 (times s)."""
    r = _r16 if f16 else (lambda t: t)
    t = scaling_layer(x, s)
    out = []
    for k, grp in enumerate(GROUPS[:n_taps]):
        if k:
            t = r(F.max_pool2d(t, 2, 2))
        for n in grp:
            t = r(F.relu(F.conv2d(t, state[f"features.{n}.weight"].to(F64), state[f"features.{n}.bias"].to(F64) * s, padding=1)))
        out.append(t)
    return out


def head(f0, f1, w, eps=EPS):
    """One tap: f0, f1 [N,C,h,w] float64, w [C] -> [N]: the mean over the pixels of sum_c w_c (f0 / (|f0| + eps) - f1 / (|f1| + eps))^2."""
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + eps)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + eps)
    return ((n0 - n1).pow(2) * w.to(F64).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def distance(x0, x1, state, s=1.0, f16=False):
    """x0, x1 [N,3,H,W] (any dtype, 0..255) -> float64 [N]: LPIPS-VGG v0.1 with normalize=False."""
    t0, t1 = taps(x0.to(F64), state, s, f16), taps(x1.to(F64), state, s, f16)
    total = torch.zeros(x0.shape[0], dtype=F64)
    for k in range(5):
        total = total + head(t0[k], t1[k], state[f"lin{k}.model.1.weight"].reshape(-1), EPS * s)
    return total


def pad8(x):
    """InputPadder, default mode: replicate-pad [N,3,H,W] to multiples of 8, the remainder split left/right and top/bottom (the smaller half first)."""
    H, W = x.shape[-2:]
    ph, pw = (((H // 8) + 1) * 8 - H) % 8, (((W // 8) + 1) * 8 - W) % 8
    return F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], mode="replicate")


def frame_lpips(edit_u8, source_u8, state, s=1.0, f16=False):
    """FrameLPIPS: uint8 [N,H,W,3] arrays of one size -> (mean, per-frame float64 array) over the frames but the last."""
    e = torch.as_tensor(np.asarray(edit_u8)).permute(0, 3, 1, 2).to(F64)
    g = torch.as_tensor(np.asarray(source_u8)).permute(0, 3, 1, 2).to(F64)
    if e.shape[0] < 2:
        raise ValueError("frame-lpips leaves the last frame out: it needs at least 2 frames")
    per = [distance(pad8(g[i:i + 1]), pad8(e[i:i + 1]), state, s, f16)[0].item() for i in range(e.shape[0] - 1)]
    per = np.array(per, dtype=np.float64)
    return float(per.mean()), per
