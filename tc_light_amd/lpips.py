"""LPIPS v0.1 with net='vgg' on the device, for the frame-lpips figure (utils/evaluation/eval_utils.py:368-386 FrameLPIPS).

The definition (lpips/lpips.py LPIPS.forward, lpips/pretrained_networks.py vgg16), per pair of images (x0, x1):
  1. ScalingLayer: (x - shift) / scale per RGB channel;
  2. torchvision VGG-16 `features` (thirteen 3x3 convolutions, padding 1, bias, ReLU; MaxPool2d(2, 2) before the last four groups), tapped after
     relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (64, 128, 256, 512, 512 channels);
  3. per tap and pixel f / (sqrt(sum_c f^2) + 1e-10) for both images, the squared difference, the 1x1 convolution `lin{k}.model.1.weight` (no bias)
     and the mean over the tap's pixels;
  4. the sum over the five taps.
The reference calls it with `normalize=False` on frames in 0..255, so the scaling layer sees 0..255; `LPIPSEngine.distance` keeps that.

Activations are NHWC f16 and the two images of a pair share one batch ([2B, H, W, C]: image 0 of pair b at row b, image 1 at row B + b).
features.0 with the scaling layer is tcl_lpips_stem_f16, the other twelve convolutions are tcl_conv3x3_f16 with the ReLU epilogue, the pools
tcl_maxpool2_f16, step 3 tcl_lpips_head and the rest tcl_lpips_finish.

f16 range.  The scaled 0..255 image reaches +-570, a hundred times the range VGG was trained on, and the network is positively homogeneous up to
its biases: relu(conv(s x) + s b) = s relu(conv(x) + b) for s > 0, and max-pooling commutes with s.  So the engine runs at a power-of-two input scale
s (INPUT_SCALE = 2^-6): s / scale_c is folded into the stem's weights and every bias is multiplied by s at load.  Every tap is then s times the
unscaled one (exactly, barring f16 subnormals) and the head's eps is eps * s, so step 3 gives the same number.  Whether a real VGG-16 checkpoint needs
this, and whether 2^-6 is the right s for it, has not been measured: no checkpoint was at hand.  What protects the figure is the head's count of
non-finite features: `distance` checks it once per call and raises FloatingPointError naming the tap.
"""
import math

import torch

from .hostlogic import pad8_amounts
from .lib import lib, stream

H16 = torch.float16
SHIFT = (-.030, -.088, -.188)                   # lpips.py ScalingLayer
SCALE = (.458, .448, .450)
GROUPS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))     # the Conv2d indices of torchvision vgg16().features, by tap
CHANNELS = (64, 128, 256, 512, 512)
TAP_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
EPS = 1e-10                                     # normalize_tensor
INPUT_SCALE = 2.0 ** -6
MIN_SIDE = 16                                   # four floor-mode pools leave at least one pixel


def vgg_param_shapes():
    shapes, ci = {}, 3
    for grp, co in zip(GROUPS, CHANNELS):
        for n in grp:
            shapes[f"features.{n}.weight"], shapes[f"features.{n}.bias"] = (co, ci, 3, 3), (co,)
            ci = co
    return shapes


def lin_param_shapes():
    return {f"lin{k}.model.1.weight": (1, c, 1, 1) for k, c in enumerate(CHANNELS)}


def seeded_state(seed=8, bias_std=0.05):
    """Stand-in weights of the right shapes (tests, plumbing; never a trained model's): He-scaled convolutions (std sqrt(2 / (9 Cin)), which keeps
    the second moment of the activations through the ReLUs) with small biases, all representable in f16, and `lin` weights |N(0, 1)| (LPIPS's are
    non-negative).  The one generator: tests and the engine draw the same tensors from a seed."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in vgg_param_shapes().items():
        std = math.sqrt(2.0 / (9 * s[1])) if k.endswith(".weight") else bias_std
        sd[k] = (torch.randn(s, generator=g) * std).to(H16).float()
    for k, s in lin_param_shapes().items():
        sd[k] = torch.randn(s, generator=g).abs()
    return sd


def check_state(state):
    """Every key LPIPS-VGG reads, with its shape, or KeyError naming the first few that are missing or mis-shaped."""
    shapes = {**vgg_param_shapes(), **lin_param_shapes()}
    bad = [k for k, s in shapes.items() if k not in state or tuple(state[k].shape) != tuple(s)]
    if bad:
        k = bad[0]
        got = tuple(state[k].shape) if k in state else "missing"
        raise KeyError(f"LPIPS state lacks or mis-shapes {len(bad)} tensors, e.g. {bad[:3]} ({k}: expected {tuple(shapes[k])}, got {got})")


def tap_sizes(H, W):
    """The (h, w) of the five taps of an H x W image: floor halving, as MaxPool2d(2, 2)."""
    return [(H >> k, W >> k) for k in range(5)]


def pad8_u8(frames):
    """Replicate-pad uint8 [N,H,W,3] frames to multiples of 8 (InputPadder.pad), staying uint8."""
    H, W = frames.shape[1:3]
    l, r, t, b = pad8_amounts(H, W)
    if not (l or r or t or b):
        return frames.contiguous()
    iy = torch.arange(-t, H + b, device=frames.device).clamp_(0, H - 1)
    ix = torch.arange(-l, W + r, device=frames.device).clamp_(0, W - 1)
    return frames.index_select(1, iy).index_select(2, ix).contiguous()


class LPIPSEngine:
    """lpips.LPIPS(net='vgg') in eval mode.  state: torchvision's `features.N.weight / .bias` and lpips' `lin{k}.model.1.weight`
    (model_utils.load_lpips_state)."""

    def __init__(self, state, device, input_scale=INPUT_SCALE):
        check_state(state)
        s = float(input_scale)
        if not (s > 0 and math.frexp(s)[0] == 0.5):
            raise ValueError(f"input_scale must be a power of two (the taps are then exactly s times the unscaled ones), got {input_scale}")
        self.dev, self.L, self.s = torch.device(device), lib(), s
        d = self.dev
        fold = (s / torch.tensor(SCALE, dtype=torch.float64)).view(1, 3, 1, 1)
        w0 = state["features.0.weight"].double() * fold                                 # [64, 3, ky, kx] -> [64, (ky, kx, c)]
        self.stem_w = w0.permute(0, 2, 3, 1).reshape(64, 27).float().contiguous().to(d)
        self.stem_b = (state["features.0.bias"].double() * s).float().contiguous().to(d)
        self.convs = {}
        for grp in GROUPS:
            for n in grp:
                if n == 0:
                    continue
                w, b = state[f"features.{n}.weight"].float(), state[f"features.{n}.bias"].double()
                co, ci = w.shape[:2]
                self.convs[n] = (w.permute(0, 2, 3, 1).reshape(co, 9 * ci).to(H16).contiguous().to(d), (b * s).to(H16).contiguous().to(d), ci, co)
        self.lin = [state[f"lin{k}.model.1.weight"].reshape(-1).float().contiguous().to(d) for k in range(5)]

    @torch.no_grad()
    def distance(self, a_u8, b_u8):
        """a_u8, b_u8 uint8 [B,H,W,3] on the device, equal sizes, H, W >= 16 -> f32 [B] (device): LPIPS(a[i], b[i]) of the 0..255 images."""
        for t in (a_u8, b_u8):
            if not (isinstance(t, torch.Tensor) and t.dim() == 4 and t.shape[-1] == 3 and t.dtype == torch.uint8 and t.is_cuda):
                raise ValueError(f"distance takes uint8 [B,H,W,3] device tensors, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if a_u8.shape != b_u8.shape:
            raise ValueError(f"the two images of a pair must have one size, got {tuple(a_u8.shape)} / {tuple(b_u8.shape)}")
        B, H, W = a_u8.shape[:3]
        if B < 1 or H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"LPIPS-VGG pools four times: it needs B >= 1 and H, W >= {MIN_SIDE}, got B = {B}, {H}x{W}")
        L, d, st = self.L, self.dev, stream()
        x = torch.cat([a_u8, b_u8]).contiguous()
        sizes = tap_sizes(H, W)
        h_P = torch.tensor([h * w for h, w in sizes], dtype=torch.int32)                # host: the head and the finish lay the workspace out from it
        ws = torch.empty(L.tcl_lpips_workspace_bytes(B, H, W), dtype=torch.uint8, device=d)
        y = torch.empty(2 * B * H * W, 64, dtype=H16, device=d)
        L.tcl_lpips_stem_f16(x, self.stem_w, self.stem_b, SHIFT[0], SHIFT[1], SHIFT[2], y, 2 * B, H, W, st)
        c = 64
        for k, grp in enumerate(GROUPS):
            h, w = sizes[k]
            if k:
                p = torch.empty(2 * B * h * w, c, dtype=H16, device=d)
                L.tcl_maxpool2_f16(y, p, 2 * B, sizes[k - 1][0], sizes[k - 1][1], c, st)
                y = p
            for n in grp:
                if n == 0:
                    continue
                wt, bias, ci, co = self.convs[n]
                o = torch.empty(2 * B * h * w, co, dtype=H16, device=d)
                L.tcl_conv3x3_f16(y, wt, bias, 0, o, 2 * B, h, w, ci, co, 1, 1, 0, 0, 3, st)
                y, c = o, co
            L.tcl_lpips_head(y, self.lin[k], B, h_P, 5, k, c, EPS * self.s, ws, st)
        out = torch.empty(B, dtype=torch.float32, device=d)
        bad = torch.empty(5, dtype=torch.int32, device=d)
        L.tcl_lpips_finish(ws, B, h_P, 5, out, bad, st)
        bad = bad.cpu().tolist()                                                        # the one host check of the call
        if any(bad):
            k = next(i for i, n in enumerate(bad) if n)
            raise FloatingPointError(f"LPIPS: {bad[k]} non-finite f16 features at tap {TAP_NAMES[k]} (counts per tap {bad}) at input scale "
                                     f"{self.s}: the activations left f16's range; build the engine with a smaller power-of-two input_scale")
        return out
