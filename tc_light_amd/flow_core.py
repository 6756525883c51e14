"""What the two optical-flow estimators (tc_light_amd.memflow, tc_light_amd.raft) share: the BasicEncoder, the on-demand correlation lookup, the weight
packing of the 1x1 and 3x3 convolutions, the seeded stand-in weights, the InputPadder rule and the engine steps both update loops are built from.

Activations are f16 NHWC rows with channel counts padded to multiples of 64 (zero weights: padded channels stay exactly 0); 1x1 convolutions are
`tcl_gemm_f16` calls, 3x3 ones the implicit-GEMM kernel, the rest lives in csrc/flow.hip.  `CorrBlock` keeps the reference's interface
(core/Networks/MemFlowNet/corr.py:74-120: `CorrBlock(fmap1, fmap2, num_levels=4, radius=4)(coords) -> [B, L*(2r+1)^2, H, W]`, NCHW f32 in and out)
but never builds the all-pairs volume: windows are computed on demand from an avg-pooled fmap2 pyramid (`tcl_corr_lookup_f32`).
"""
import ctypes

import numpy as np
import torch

from .hostlogic import pad8_amounts
from .lib import lib, stream

H16 = torch.float16


# ------------------------------------------------------------------------------------------------ parameter shapes / seeded stand-ins
def encoder_param_shapes(prefix, norm, output_dim=256):
    """State-dict keys of BasicEncoder(output_dim, norm_fn) (cnn.py:124-189) under `prefix` ('fnet.' / 'cnet.')."""
    sh = {}

    def nrm(p, c):
        if norm == "batch":
            for k in ("weight", "bias", "running_mean", "running_var"):
                sh[p + k] = (c,)
            sh[p + "num_batches_tracked"] = ()

    sh[prefix + "conv1.weight"] = (64, 3, 7, 7); sh[prefix + "conv1.bias"] = (64,)
    nrm(prefix + "norm1.", 64)
    cin = 64
    for li, (dim, stride) in enumerate(((64, 1), (96, 2), (128, 2)), 1):
        for bi, (ci, st) in enumerate(((cin, stride), (dim, 1))):
            p = f"{prefix}layer{li}.{bi}."
            sh[p + "conv1.weight"] = (dim, ci, 3, 3); sh[p + "conv1.bias"] = (dim,)
            sh[p + "conv2.weight"] = (dim, dim, 3, 3); sh[p + "conv2.bias"] = (dim,)
            nrm(p + "norm1.", dim); nrm(p + "norm2.", dim)
            if st != 1:
                nrm(p + "norm3.", dim)
                sh[p + "downsample.0.weight"] = (dim, ci, 1, 1); sh[p + "downsample.0.bias"] = (dim,)
                nrm(p + "downsample.1.", dim)                      # the same module as norm3 (cnn.py:42-43): duplicated keys
        cin = dim
    sh[prefix + "conv2.weight"] = (output_dim, 128, 1, 1); sh[prefix + "conv2.bias"] = (output_dim,)
    return sh


def seeded_state_dict(shapes, seed):
    """Seeded stand-in weights (no checkpoint in the image): He-scaled convs, BatchNorm statistics near identity; the duplicated
    `downsample.1.*` entries repeat `norm3.*`."""
    g = np.random.default_rng(seed)
    sd = {}
    for k, s in shapes.items():
        if ".downsample.1." in k:
            continue
        if k.endswith("rel_ind"):                                               # RelPosEmb buffer (gma.py:16-18), unused at inference
            n = s[0]
            sd[k] = torch.arange(n).view(1, -1) - torch.arange(n).view(-1, 1) + n - 1
        elif k.endswith("gamma"):                                               # zero-initialised in the reference; non-zero so the memory read matters
            sd[k] = torch.tensor([0.5])
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(1, dtype=torch.int64)
        elif k.endswith("running_var"):
            sd[k] = torch.from_numpy((0.5 + g.random(s)).astype(np.float32))
        elif k.endswith("running_mean") or k.endswith("bias"):
            sd[k] = torch.from_numpy(((0.002 if "flow_head.ffn2.2" in k else 0.1) * g.standard_normal(s)).astype(np.float32))
        elif len(s) == 1:                                                      # norm weight
            sd[k] = torch.from_numpy((0.8 + 0.4 * g.random(s)).astype(np.float32))
        else:
            fan = int(np.prod(s[1:]))
            gain = (1.0 / fan) ** 0.5 if (".ffn" in k or ".pw." in k or ".conv_list." in k) else (2.0 / fan) ** 0.5   # residual branches: keep 15 iterations tame
            if "flow_head.ffn2.2" in k:
                gain *= 0.02                                                    # small flow updates: the 15 GRU iterations stay bounded
            sd[k] = torch.from_numpy((g.standard_normal(s) * gain).astype(np.float32))
    for k in shapes:
        if ".downsample.1." in k:
            sd[k] = sd[k.replace(".downsample.1.", ".norm3.")]
    return sd


# ------------------------------------------------------------------------------------------------ weight packing, padding
def pad_to(t, dim, n):
    """`t` with zeros appended along `dim` up to size n."""
    if t.shape[dim] == n:
        return t
    shp = list(t.shape); shp[dim] = n - t.shape[dim]
    return torch.cat([t, torch.zeros(shp, dtype=t.dtype)], dim)


def up64(c):
    return (c + 63) // 64 * 64


class Lin:
    """1x1 convolution as a GEMM over channel-padded f16 rows: weight [co64, ci64] (zero rows / columns for the padding), bias [co64]
    (zero when `b` is None)."""

    def __init__(self, w, b, dev):
        co, ci = w.shape[0], w.shape[1]
        self.ci, self.co = up64(ci), up64(co)
        self.w = pad_to(pad_to(w.reshape(co, ci), 0, self.co), 1, self.ci).to(H16).contiguous().to(dev)
        self.b = pad_to(b if b is not None else torch.zeros(co), 0, self.co).to(H16).contiguous().to(dev)


def conv3_weights(w, b, co_pad, ci_pad=None):
    """3x3 conv weights [co, ci, 3, 3] f32 for tcl_conv3x3_f16 -> (weight [co_pad, 9*ci_pad] f16 tap-major: column (ky*3 + kx)*ci_pad + c,
    bias [co_pad] f16, ci_pad, co_pad), zero rows / columns / bias entries for the padding.  ci_pad None: the input channels as they are."""
    ci_pad = ci_pad or w.shape[1]
    w = pad_to(pad_to(w, 0, co_pad), 1, ci_pad)
    return w.permute(0, 2, 3, 1).reshape(co_pad, 9 * ci_pad).to(H16).contiguous(), pad_to(b, 0, co_pad).to(H16).contiguous(), ci_pad, co_pad


def pad8(x):
    """eval_utils.InputPadder: replicate-pad H, W of [..., H, W] up to multiples of 8, split evenly -> (padded, [left, right, top, bottom])."""
    pad = list(pad8_amounts(*x.shape[-2:]))
    return torch.nn.functional.pad(x, pad, mode="replicate"), pad


# ------------------------------------------------------------------------------------------------ engine steps
class FlowEngine:
    """The steps both estimators and their encoders are made of, on `self.dev` through `self.L`."""

    def __init__(self, device):
        self.dev, self.L = torch.device(device), lib()

    def _conv3w(self, w, b, co_pad, ci_pad=None):
        w, b, ci, co = conv3_weights(w, b, co_pad, ci_pad)
        return w.to(self.dev), b.to(self.dev), ci, co

    def _gemm(self, x, lin, M, act=0, resid=None, lda=None):
        y = torch.empty(M, lin.co, dtype=H16, device=self.dev)
        self.L.tcl_gemm_f16(x, lin.w, lin.b, resid if resid is not None else 0, y, M, lin.co, lin.ci, lda or lin.ci, lin.ci, lin.co, lin.co, act, stream())
        return y

    def _c3(self, x, spec, B, h, w, relu, stride=1):
        """3x3 convolution (padding 1) of rows [B*h*w, ci] with a `conv3_weights` spec -> rows [B*ho*wo, co]."""
        wt, b, ci, co = spec
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        y = torch.empty(B * ho * wo, co, dtype=H16, device=self.dev)
        self.L.tcl_conv3x3_f16(x, wt, b, 0, y, B, h, w, ci, co, stride, 1, 0, 0, 3 if relu else 0, stream())
        return y

    def coords_grid(self, B, h, w):
        """[B,2,h,w] f32: channel 0 = x, channel 1 = y of every pixel."""
        ys, xs = torch.meshgrid(torch.arange(h, device=self.dev).float(), torch.arange(w, device=self.dev).float(), indexing="ij")
        return torch.stack([xs, ys])[None].expand(B, 2, h, w).contiguous()

    def _context_split(self, c, P):
        """cnet rows [P,256] -> net = tanh(c[:, :128]), inp = relu(c[:, 128:])."""
        net = torch.empty(P, 128, dtype=H16, device=self.dev); inp = torch.empty(P, 128, dtype=H16, device=self.dev)
        self.L.tcl_context_split_f16(c, net, inp, P, stream())
        return net, inp

    def _upsample(self, net, coords0, coords1, B, h, w):
        """The mask head (self.mask0 3x3 + ReLU, self.mask2 1x1) on the last hidden state and the convex 8x up-sampling -> (flow_low, flow_up)."""
        mask = self._gemm(self._c3(net, self.mask0, B, h, w, True), self.mask2, B * h * w)      # [P,576]; the 0.25 factor is applied in the kernel
        flow_low = coords1 - coords0
        up = torch.empty(B, 2, 8 * h, 8 * w, dtype=torch.float32, device=self.dev)
        self.L.tcl_upsample_flow_f32(flow_low.contiguous(), mask, 576, 0.25, up, B, h, w, stream())
        return flow_low, up


class EncoderEngine(FlowEngine):
    """BasicEncoder (cnn.py:124-216) in f16 NHWC: 7x7 stem kernel, implicit-GEMM 3x3 convs, 1x1 convs as GEMMs.  norm 'batch' (cnet):
    eval BatchNorm folded into the conv weights / bias, ReLU in the GEMM epilogue; norm 'instance' (fnet): tcl_instnorm_f16.  Channel
    counts are padded to multiples of 64 with zero weights (96 -> 128); padded channels stay exactly 0 through norm and ReLU.
    `f32_stem` (instance norm only): the stem convolution stays in f32 up to the normalisation (tcl_conv7x7s2_instnorm_f16)."""

    def __init__(self, sd, prefix, norm, device, f32_stem=False):
        super().__init__(device)
        self.norm, self.f32_stem = norm, f32_stem
        f = {k[len(prefix):]: v.float() for k, v in sd.items() if k.startswith(prefix) and v.dtype.is_floating_point}

        def fold(wk, bk, nk):
            w, b = f[wk], f[bk]
            if norm == "batch":
                s = f[nk + "weight"] / torch.sqrt(f[nk + "running_var"] + 1e-5)
                w = w * s.view(-1, 1, 1, 1)
                b = (b - f[nk + "running_mean"]) * s + f[nk + "bias"]
            return w, b

        w, b = fold("conv1.weight", "conv1.bias", "norm1.")
        self.stem = (w.reshape(64, 147).t().contiguous().to(self.dev), b.contiguous().to(self.dev))
        self.blocks = []
        for li, stride in ((1, 1), (2, 2), (3, 2)):
            for bi in (0, 1):
                p = f"layer{li}.{bi}."
                blk = dict(stride=stride if bi == 0 else 1)
                for cn, nn_ in (("conv1", "norm1."), ("conv2", "norm2.")):
                    w, b = fold(p + cn + ".weight", p + cn + ".bias", p + nn_)
                    blk[cn] = self._conv3w(w, b, up64(w.shape[0]), up64(w.shape[1]))
                if blk["stride"] != 1:
                    blk["down"] = Lin(*fold(p + "downsample.0.weight", p + "downsample.0.bias", p + "norm3."), self.dev)
                self.blocks.append(blk)
        self.out = Lin(f["conv2.weight"], f["conv2.bias"], self.dev)
        self._ws = {}

    def _inorm(self, x, B, HW, C, relu):
        key = (B, C)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(self.L.tcl_instnorm_workspace_bytes(B, C), dtype=torch.uint8, device=self.dev)
        y = torch.empty_like(x)
        self.L.tcl_instnorm_f16(x, y, B, HW, C, 1e-5, int(relu), ws, stream())
        return y

    def _stem(self, img):
        """conv1 + norm1 + relu1 -> f16 rows [B*h*w, 64], h, w."""
        B, _, H, W = img.shape
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x = torch.empty(B * h * w, 64, dtype=H16, device=self.dev)
        if self.f32_stem:
            ws = torch.empty(self.L.tcl_stem_instnorm_workspace_bytes(B, H, W), dtype=torch.uint8, device=self.dev)
            self.L.tcl_conv7x7s2_instnorm_f16(img.float().contiguous(), self.stem[0], self.stem[1], x, B, H, W, 1e-5, ws, stream())
            return x, h, w
        bn = self.norm == "batch"
        self.L.tcl_conv7x7s2_c3_f16(img.float().contiguous(), self.stem[0], self.stem[1], x, B, H, W, int(bn), stream())
        if not bn:
            x = self._inorm(x, B, h * w, 64, True)
        return x, h, w

    @torch.no_grad()
    def forward(self, img):
        """img [B,3,H,W] f32 (H, W multiples of 8) -> feature map [B*(H/8)*(W/8), 256] f16 (NHWC rows), (H/8, W/8)."""
        L, bn = self.L, self.norm == "batch"
        B = img.shape[0]
        x, h, w = self._stem(img)
        for blk in self.blocks:
            st = blk["stride"]
            h2, w2 = (h - 1) // st + 1, (w - 1) // st + 1
            C = blk["conv1"][3]
            y = self._c3(x, blk["conv1"], B, h, w, bn, st)
            if not bn:
                y = self._inorm(y, B, h2 * w2, C, True)
            y = self._c3(y, blk["conv2"], B, h2, w2, bn)
            if not bn:
                y = self._inorm(y, B, h2 * w2, C, True)
            if st != 1:
                Cin = x.shape[1]
                xs = torch.empty(B * h2 * w2, Cin, dtype=H16, device=self.dev)
                L.tcl_subsample2_nhwc_f16(x, xs, B, h, w, Cin, stream())
                xd = self._gemm(xs, blk["down"], B * h2 * w2)
                x = xd if bn else self._inorm(xd, B, h2 * w2, C, False)
            out = torch.empty_like(y)
            L.tcl_add_act_f16(x, y, out, y.numel(), 3, stream())
            x, h, w = out, h2, w2
        return self._gemm(x, self.out, B * h * w), (h, w)


class CorrBlock:
    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        if not fmap1.is_cuda:
            raise RuntimeError("tc_light_amd.flow_core.CorrBlock needs device tensors (no CPU path)")
        self.num_levels, self.radius = num_levels, radius
        B, D, H, W = fmap1.shape
        self.shape = (B, D, H, W)
        L = lib()
        self.f1 = fmap1.float().permute(0, 2, 3, 1).contiguous()
        lv = [fmap2.float().permute(0, 2, 3, 1).contiguous()]
        hs, ws = [H], [W]
        for _ in range(num_levels - 1):
            h, w = hs[-1] // 2, ws[-1] // 2
            if h < 1 or w < 1:
                raise ValueError("feature map too small for the requested number of pyramid levels")
            nxt = torch.empty(B, h, w, D, dtype=torch.float32, device=fmap1.device)
            L.tcl_avgpool2_nhwc_f32(lv[-1], nxt, B, hs[-1], ws[-1], D, stream())
            lv.append(nxt); hs.append(h); ws.append(w)
        self.levels = lv
        # f16 copies for the tile-sharing lookup (tcl_corr_lookup_rows_tiled_f16): level 0 came out of the encoder in f16, so this is its exact value;
        # the pooled levels are rounded once (f32 pooling chain above)
        self.f1h, self.levels_h = self.f1.half(), [t.half() for t in lv]
        self._ptrs_h = (ctypes.c_void_p * num_levels)(*[t.data_ptr() for t in self.levels_h])
        self._flags = torch.zeros(num_levels * ((H + 7) // 8) * ((W + 7) // 8), dtype=torch.int32, device=fmap1.device)
        self._ptrs = (ctypes.c_void_p * num_levels)(*[t.data_ptr() for t in lv])
        self._hs = (ctypes.c_int * num_levels)(*hs)
        self._ws = (ctypes.c_int * num_levels)(*ws)

    @classmethod
    def from_nhwc(cls, f1, f2, num_levels=4, radius=4):
        """f1, f2 [B,H,W,D] f32 NHWC on the device."""
        return cls(f1.permute(0, 3, 1, 2), f2.permute(0, 3, 1, 2), num_levels, radius)

    def lookup_rows(self, coords, out_rows, tiled=True):
        """Window lookup written as f16 rows [B*H*W, ld] (first L*(2r+1)^2 channels) for the motion encoder's GEMM.  `tiled`: the kernel that shares
        neighbour rows between 8 x 8 pixel tiles (one entry, radius 4 only; profiles/r6_ab_corr_tiled.txt); else, and otherwise, the per-pixel one."""
        B, D, H, W = self.shape
        if tiled and B == 1 and self.radius == 4:
            lib().tcl_corr_lookup_rows_tiled_f16(self.f1h, self._ptrs_h, self.f1, self._ptrs, self._hs, self._ws, self.num_levels, coords, out_rows,
                                                 out_rows.shape[1], H, W, D, self.radius, self._flags, stream())
            return
        lib().tcl_corr_lookup_rows_f16(self.f1, self._ptrs, self._hs, self._ws, self.num_levels, coords, out_rows, out_rows.shape[1], B, H, W, D,
                                       self.radius, stream())

    def __call__(self, coords):
        B, D, H, W = self.shape
        n = 2 * self.radius + 1
        out = torch.empty(B, self.num_levels * n * n, H, W, dtype=torch.float32, device=coords.device)
        lib().tcl_corr_lookup_f32(self.f1, self._ptrs, self._hs, self._ws, self.num_levels, coords.float().contiguous(), out, B, H, W, D,
                                  self.radius, 1, stream())
        return out
