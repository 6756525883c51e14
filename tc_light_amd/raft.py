"""RAFT inference on the device: the second flow estimator of the stage-2 inputs (`data.flow_model: raft`).

`RAFTEngine` = the reference's RAFT (utils/evaluation/core/raft.py:73-131, not small, no alternate_corr, no mixed precision) with
`forward(test_mode=True)` semantics.  The two BasicEncoders, the correlation lookup and the engine steps are the ones MemFlowNet uses
(tc_light_amd.flow_core: the keys, shapes and the CorrBlock are the same); the fnet stem keeps its convolution in f32 up to the instance norm
(tcl_conv7x7s2_instnorm_f16), because the stage-2 frames reach RAFT in [0, 1] rather than [0, 255] (see `estimate_flows_raft`) and the f16 rounding
of the stem would then be amplified by the normalisation.  The update block (update.py:60-136) runs on f16 NHWC rows: convc1 / mask.2 as GEMMs, the 3x3 convolutions on the implicit-GEMM
kernel, convf1 (7x7 over the 2-channel flow) in csrc/raft.hip, and each SepConvGRU half-step as two fused kernels (gate: [z | r] + r*h;
candidate: q + the blend, in place).  The GRU input is x = [inp | motion] and `inp` is the same on every iteration: its share of the six
convolutions (with their biases) is computed once per pair as an f32 per-pixel bias (the "context fold"), so the per-iteration K is 1 280.
Pairs are independent (no memory between them): `estimate_flows_raft` encodes every frame once and runs the pairs in batches.
Pinned against the reference by tests/golden/raft.npz (tests/test_gpu_raft.py).
"""
import torch

from . import flow_core
from .flow_core import H16, CorrBlock, EncoderEngine, FlowEngine, Lin, encoder_param_shapes
from .lib import stream

ITERS = 20                                                              # video_dataparser.py:149


def raft_param_shapes():
    """State-dict keys of RAFT(small=False) (raft.py:40-43, extractor.py:117-141, update.py:60-136), without the DataParallel `module.` prefix."""
    sh = {}
    sh.update(encoder_param_shapes("fnet.", "instance"))
    sh.update(encoder_param_shapes("cnet.", "batch"))
    u = "update_block."

    def conv(name, co, ci, kh, kw):
        sh[u + name + ".weight"] = (co, ci, kh, kw); sh[u + name + ".bias"] = (co,)

    conv("encoder.convc1", 256, 324, 1, 1); conv("encoder.convc2", 192, 256, 3, 3)
    conv("encoder.convf1", 128, 2, 7, 7); conv("encoder.convf2", 64, 128, 3, 3)
    conv("encoder.conv", 126, 256, 3, 3)
    for d, (kh, kw) in (("1", (1, 5)), ("2", (5, 1))):
        for g in "zrq":
            conv(f"gru.conv{g}{d}", 128, 384, kh, kw)
    conv("flow_head.conv1", 256, 128, 3, 3); conv("flow_head.conv2", 2, 256, 3, 3)
    conv("mask.0", 256, 128, 3, 3); conv("mask.2", 576, 256, 1, 1)
    return sh


def seeded_state_dict(seed=5):
    """Seeded stand-in weights: flow_core.seeded_state_dict's rules (He-scaled convs, BatchNorm statistics near identity), with
    update_block.flow_head.conv2 scaled down so that 20 iterations stay bounded."""
    sd = flow_core.seeded_state_dict(raft_param_shapes(), seed)
    for k in ("update_block.flow_head.conv2.weight", "update_block.flow_head.conv2.bias"):
        sd[k] = sd[k] * 0.05
    return sd


def gru_taps(w):
    """SepConvGRU weight [co, 384, 1, 5] / [co, 384, 5, 1] -> [co, tap, ci] with ci = h | inp | motion."""
    return w.reshape(w.shape[0], 384, 5).permute(0, 2, 1)


def gru_hm_weight(t):
    """[co, 5, 384] -> [co, 1280]: the (h or r*h) | motion share, column tap*256 + src*128 + c (the layout tcl_raft_sepconv_f16 reads at C1 = 128)."""
    return torch.cat([t[:, :, :128], t[:, :, 256:]], 2).reshape(t.shape[0], 1280)


def gru_ctx_weight(t):
    """[co, 5, 384] -> [co, 640]: the inp share, column tap*128 + c (C1 = 0)."""
    return t[:, :, 128:256].reshape(t.shape[0], 640)


def convf1_weight_t(w):
    """[128, 2, 7, 7] -> w_t [98, 128] with row c*49 + ky*7 + kx."""
    return w.reshape(128, 98).t().contiguous()


def check_size(H, W):
    """The working size RAFT can take here: InputPadder pads to multiples of 8 and the raft branch of load_flow never unpads (so only sizes the
    padder leaves alone are served), and the coarsest correlation level must be at least 2 x 2 (bilinear_sampler divides by W - 1)."""
    if H % 8 or W % 8:
        raise ValueError(f"RAFT needs a working size divisible by 8 (the reference pads and never unpads the raft flows), got {H}x{W}")
    if H // 64 < 2 or W // 64 < 2:
        raise ValueError(f"RAFT needs H/64 >= 2 and W/64 >= 2 (a 1-pixel coarsest correlation level gives NaN in the reference), got {H}x{W}")


class RAFTEngine(FlowEngine):
    """RAFT (raft.py:73-131) on the device for B >= 1 independent pairs."""

    def __init__(self, state_dict, device, iters=ITERS):
        missing = [k for k in raft_param_shapes() if k not in state_dict]
        if missing:
            raise KeyError(f"RAFT state dict lacks {len(missing)} keys, e.g. {missing[:3]}")
        super().__init__(device)
        d, self.iters = self.dev, iters
        self.fnet = EncoderEngine(state_dict, "fnet.", "instance", d, f32_stem=True)
        self.cnet = EncoderEngine(state_dict, "cnet.", "batch", d)
        f = {k[len("update_block."):]: v.float() for k, v in state_dict.items() if k.startswith("update_block.")}
        self.convc1 = Lin(f["encoder.convc1.weight"], f["encoder.convc1.bias"], d)                       # 324 -> 384 padded input channels
        self.convc2 = self._conv3w(f["encoder.convc2.weight"], f["encoder.convc2.bias"], 192)
        self.convf1 = (convf1_weight_t(f["encoder.convf1.weight"]).to(d), f["encoder.convf1.bias"].contiguous().to(d))
        self.convf2 = self._conv3w(f["encoder.convf2.weight"], f["encoder.convf2.bias"], 64)
        self.conv = self._conv3w(f["encoder.conv.weight"], f["encoder.conv.bias"], 128)                       # 126 + 2 zero channels (the flow goes there)
        self.gru = []
        for dn in ("1", "2"):
            taps = lambda g: gru_taps(f[f"gru.conv{g}{dn}.weight"])                                      # [co, tap, ci]: ci = h | inp | motion
            zr, q = torch.cat([taps("z"), taps("r")]), taps("q")
            hm = lambda t: gru_hm_weight(t).to(H16).contiguous().to(d)                                    # (h or r*h) | motion
            ctx = lambda t: gru_ctx_weight(t).to(H16).contiguous().to(d)                                  # the inp share

            bzr = torch.cat([f[f"gru.convz{dn}.bias"], f[f"gru.convr{dn}.bias"]]).contiguous().to(d)
            self.gru.append(dict(w_zr=hm(zr), w_q=hm(q), c_zr=ctx(zr), c_q=ctx(q), b_zr=bzr, b_q=f[f"gru.convq{dn}.bias"].contiguous().to(d)))
        self.fh1 = self._conv3w(f["flow_head.conv1.weight"], f["flow_head.conv1.bias"], 256)
        self.fh2 = self._conv3w(f["flow_head.conv2.weight"], f["flow_head.conv2.bias"], 64)                  # 2 channels + zero padding
        self.mask0 = self._conv3w(f["mask.0.weight"], f["mask.0.bias"], 256)
        self.mask2 = Lin(f["mask.2.weight"], f["mask.2.bias"], d)

    # ---- building blocks
    def context_fold(self, inp, B, h, w):
        """The inp share of the six GRU convolutions + their biases, f32 per pixel: [(gate [P,256], cand [P,128]) for the 1x5 and the 5x1 half]."""
        P, out = B * h * w, []
        for di, g in enumerate(self.gru):
            pair = []
            for wk, bk, n in (("c_zr", "b_zr", 256), ("c_q", "b_q", 128)):
                y = torch.empty(P, n, dtype=torch.float32, device=self.dev)
                self.L.tcl_raft_sepconv_f16(inp, 0, 0, g[wk], g[bk], 0, y, 0, 0, 0, B, h, w, n, di, 0, stream())
                pair.append(y)
            out.append(tuple(pair))
        return out

    def gru_half(self, di, net, mf, fold, z, rh, B, h, w):
        """One SepConvGRU half (update.py:43-48 / :51-56): net updated in place."""
        g, L = self.gru[di], self.L
        L.tcl_raft_sepconv_f16(net, mf, 128, g["w_zr"], 0, fold[0], 0, z, rh, net, B, h, w, 256, di, 1, stream())
        L.tcl_raft_sepconv_f16(rh, mf, 128, g["w_q"], 0, fold[1], 0, z, 0, net, B, h, w, 128, di, 2, stream())

    # ---- the network
    @torch.no_grad()
    def encode(self, images):
        """images [B,3,H,W] already normalised to RAFT's [-1, 1] input -> (fmap rows [B*h*w, 256] f16, context rows [B*h*w, 256] f16, (h, w))."""
        fm, hw = self.fnet.forward(images)
        c, _ = self.cnet.forward(images)
        return fm, c, hw

    @torch.no_grad()
    def forward(self, image1, image2, iters=None, flow_init=None):
        """RAFT.forward(image1, image2, iters, flow_init, test_mode=True): images [B,3,H,W] in [0, 255] -> (flow_low [B,2,H/8,W/8], flow_up [B,2,H,W])."""
        B, _, H, W = image1.shape
        check_size(H, W)
        x = torch.cat([image1, image2]).to(self.dev).float()
        x = 2 * (x / 255.0) - 1.0
        fm, hw = self.fnet.forward(x)
        c, _ = self.cnet.forward(x[:B])
        P = hw[0] * hw[1]
        return self.refine(fm[:B * P], fm[B * P:], c, B, hw, iters, flow_init)

    @torch.no_grad()
    def refine(self, f1, f2, c, B, hw, iters=None, flow_init=None):
        """The iterations of raft.py:101-131 on encoded pairs: f1 / f2 / c rows [B*h*w, 256] f16 -> (flow_low, flow_up)."""
        L, d = self.L, self.dev
        h, w = hw
        P = B * h * w
        iters = self.iters if iters is None else iters
        # one CorrBlock per pair: the lookup that shares neighbour rows between 8 x 8 pixel tiles serves one entry at a time
        f1, f2 = f1.float().view(B, h, w, 256), f2.float().view(B, h, w, 256)
        corrs = [CorrBlock.from_nhwc(f1[j:j + 1], f2[j:j + 1]) for j in range(B)]
        net, inp = self._context_split(c, P)
        fold = self.context_fold(inp, B, h, w)
        coords0 = self.coords_grid(B, h, w)
        coords1 = coords0.clone() if flow_init is None else (coords0 + flow_init.to(d).float()).contiguous()
        corr_rows = torch.zeros(P, 384, dtype=H16, device=d)              # 324 channels + zero padding
        fl1 = torch.empty(P, 128, dtype=H16, device=d)
        cf = torch.empty(P, 256, dtype=H16, device=d)
        z = torch.empty(P, 128, dtype=torch.float32, device=d)
        rh = torch.empty(P, 128, dtype=H16, device=d)
        for _ in range(iters):
            for j, corr in enumerate(corrs):
                corr.lookup_rows(coords1[j:j + 1], corr_rows[j * h * w:(j + 1) * h * w])
            flow = coords1 - coords0
            cor = self._c3(self._gemm(corr_rows, self.convc1, P, act=3), self.convc2, B, h, w, True)          # [P,192]
            L.tcl_raft_convf1_f16(coords1, self.convf1[0], self.convf1[1], fl1, 128, B, h, w, stream())
            flo = self._c3(fl1, self.convf2, B, h, w, True)                                                     # [P,64]
            L.tcl_concat_channels_f16(cor, 192, flo, 64, cf, P, stream())
            mf = self._c3(cf, self.conv, B, h, w, True)                                                         # [P,128]: 126 + 2
            L.tcl_nchw_f32_to_rows_f16(flow, mf, B, 2, h * w, 128, 126, 0, stream())                           # cat([out, flow]) (update.py:90)
            self.gru_half(0, net, mf, fold[0], z, rh, B, h, w)
            self.gru_half(1, net, mf, fold[1], z, rh, B, h, w)
            delta = self._c3(self._c3(net, self.fh1, B, h, w, True), self.fh2, B, h, w, False)               # [P,64]: 2 + zero padding
            L.tcl_rows_f16_to_nchw_f32(delta, coords1, B, 2, h * w, 64, 0, 1.0, 1.0, stream())
        # the mask of the last iteration only (the reference computes it on every one and returns the last up-sampling)
        return self._upsample(net, coords0, coords1, B, h, w)


def useful_flops(H, W, iters=ITERS):
    """Multiply-adds x 2 of one pair at H x W as the reference runs it once (two fnet passes, one cnet pass, `iters` update blocks with the
    context term folded, the mask head once).  `corr_volume` is the reference's all-pairs matmul, which this engine never computes (the windows are
    evaluated on demand), so it is not part of `total`."""
    hh, ww = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    enc = 2 * hh * ww * 64 * 147                                         # stem
    cin = 64
    for dim, stride in ((64, 1), (96, 2), (128, 2)):
        hh, ww = (hh - 1) // stride + 1, (ww - 1) // stride + 1
        px = 2 * hh * ww * dim
        enc += px * 9 * cin + 3 * px * 9 * dim + (px * cin if stride != 1 else 0)  # block 0: conv1, conv2 (+ 1x1 shortcut); block 1: two convs
        cin = dim
    enc += 2 * hh * ww * 256 * 128                                       # conv2 (1x1)
    P = (H // 8) * (W // 8)
    it = 2 * P * (324 * 256 + 256 * 192 * 9 + 98 * 128 + 128 * 64 * 9 + 256 * 126 * 9 + 2 * 5 * 256 * 384 + 128 * 256 * 9 + 256 * 2 * 9)
    fold = 2 * P * 2 * 5 * 128 * 384
    mask = 2 * P * (128 * 256 * 9 + 256 * 576)
    corr = 2 * P * P * 256
    return dict(encoders=3 * enc, update=iters * it, fold=fold, mask=mask, corr_volume=corr, total=3 * enc + iters * it + fold + mask)


def estimate_flows_raft(engine, frames, batch=4):
    """VideoDataParser.load_flow / calc_flow for flow_model 'raft' (video_dataparser.py:63-124, 141-156): frames [N,3,H,W] in [0, 1] ->
    (future_flows, past_flows) [N,2,H,W] f32 on the device; the last future flow and the first past flow are zero; 20 iterations, no warm start.

    The reference hands RAFT the [0, 1] frames as they are (only the memflow branch rescales them, :77-78) and RAFT normalises as if they were
    0-255 images: its inputs lie in [-1, -0.992].  The cache must hold what the reference would write, so this reproduces that.  fnet and cnet
    run once per frame (the reference: once per pair and direction); source frame i's context serves both of its pairs; pairs run `batch` at a time."""
    check_size(*frames.shape[-2:])
    N = frames.shape[0]
    d = engine.dev
    x = 2 * (frames.to(d).float() / 255.0) - 1.0
    fms, cs = [], []
    for s in range(0, N, max(batch, 1)):
        fm, c, hw = engine.encode(x[s:s + batch])
        fms.append(fm); cs.append(c)
    P = hw[0] * hw[1]
    fm = torch.cat(fms).view(N, P, 256); c = torch.cat(cs).view(N, P, 256)
    pairs = [(i, i + 1, True) for i in range(N - 1)] + [(i, i - 1, False) for i in range(1, N)]
    fut = torch.zeros(N, 2, *frames.shape[-2:], device=d); past = torch.zeros_like(fut)
    for s in range(0, len(pairs), max(batch, 1)):
        grp = pairs[s:s + batch]
        src = torch.tensor([p[0] for p in grp], device=d); tgt = torch.tensor([p[1] for p in grp], device=d)
        _, up = engine.refine(fm[src].reshape(-1, 256), fm[tgt].reshape(-1, 256), c[src].reshape(-1, 256), len(grp), hw)
        for j, (i, _, is_future) in enumerate(grp):
            (fut if is_future else past)[i] = up[j]
    return fut, past
