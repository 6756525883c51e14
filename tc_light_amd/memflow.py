"""MemFlowNet inference on the device (SURVEY 8(f) rank 2 -- the flow estimator that produces the stage-2 inputs).

`MemFlowEngine` = the reference's MemFlowNet (things_memflownet: BasicEncoder fnet / cnet, GMA-SK2 update block, `InferenceCore` + `MemoryManager`,
utils/evaluation/memflow/...; inference_core_skflow.py:20-54) on f16 NHWC activations.  The encoders, the correlation lookup, the weight packing and
the engine steps it shares with RAFT are tc_light_amd.flow_core's; here are the GMA-SK2 update block (depthwise 15x15 / 7x7 convolutions fused with
residual + GELU in csrc/flow.hip), the memory read on the flash kernel (head_dim 128) and the working memory.
`estimate_flows` reproduces VideoDataParser.load_flow (interleaved future / past pairs on one inference core, per-direction warm start).
Pinned against the reference modules by tests/golden/memflow_*.npz (tests/test_gpu_memflow.py).
"""
import numpy as np
import torch

from .flow_core import H16, CorrBlock, EncoderEngine, FlowEngine, Lin, encoder_param_shapes, pad8, pad_to, seeded_state_dict, up64  # noqa: F401 (re-exports)
from .hostlogic import memflow_splitkv_chunks
from .lib import stream


# ------------------------------------------------------------------------------------------------ parameter shapes
def pcblock_param_shapes(p, cin, cout, k_conv):
    """PCBlock4_Deep_nopool_res(C_in, C_out, k_conv) (sk2.py:6-22)."""
    mid = int(1.5 * cin)
    sh = {}
    for i, k in enumerate(k_conv):
        sh[p + f"conv_list.{i}.weight"] = (cin, 1, k, k); sh[p + f"conv_list.{i}.bias"] = (cin,)
    sh[p + "ffn1.0.weight"] = (mid, cin, 1, 1); sh[p + "ffn1.0.bias"] = (mid,)
    sh[p + "ffn1.2.weight"] = (cin, mid, 1, 1); sh[p + "ffn1.2.bias"] = (cin,)
    sh[p + "pw.weight"] = (cin, cin, 1, 1); sh[p + "pw.bias"] = (cin,)
    sh[p + "ffn2.0.weight"] = (mid, cin, 1, 1); sh[p + "ffn2.0.bias"] = (mid,)
    sh[p + "ffn2.2.weight"] = (cout, mid, 1, 1); sh[p + "ffn2.2.bias"] = (cout,)
    return sh


K_CONV, K_GRU = (1, 15), (1, 7)                                  # sk2.py:201-202


def memflow_param_shapes():
    """State-dict keys of MemFlowNet(cfg = things_memflownet: basicencoder cnet/fnet, GMA-SK2) (MemFlow.py:21-64)."""
    sh = {}
    sh.update(encoder_param_shapes("cnet.", "batch"))
    sh.update(encoder_param_shapes("fnet.", "instance"))
    u = "update_block."
    sh.update(pcblock_param_shapes(u + "encoder.convc1.", 324, 256, K_CONV))
    sh.update(pcblock_param_shapes(u + "encoder.convc2.", 256, 192, K_CONV))
    sh[u + "encoder.convf1.weight"] = (128, 2, 1, 1); sh[u + "encoder.convf1.bias"] = (128,)
    sh.update(pcblock_param_shapes(u + "encoder.convf2.", 128, 64, K_CONV))
    sh.update(pcblock_param_shapes(u + "encoder.conv.", 256, 126, K_CONV))
    sh.update(pcblock_param_shapes(u + "gru.", 512, 128, K_GRU))
    sh.update(pcblock_param_shapes(u + "flow_head.", 128, 2, K_CONV))
    sh[u + "mask.0.weight"] = (256, 128, 3, 3); sh[u + "mask.0.bias"] = (256,)
    sh[u + "mask.2.weight"] = (576, 256, 1, 1); sh[u + "mask.2.bias"] = (576,)
    sh[u + "aggregator.to_v.weight"] = (128, 128, 1, 1); sh[u + "aggregator.gamma"] = (1,)
    sh["att.to_qk.weight"] = (256, 128, 1, 1)
    sh["att.pos_emb.rel_height.weight"] = (319, 128); sh["att.pos_emb.rel_width.weight"] = (319, 128)
    sh["att.pos_emb.rel_ind"] = (160, 160)
    return sh


# ------------------------------------------------------------------------------------------------ update block + inference core
class _PCBlock:
    """PCBlock4_Deep_nopool_res (sk2.py:6-30): x = gelu(x + ffn1(x)); x = gelu(x + dw_k(x)) for k in k_conv; x = gelu(x + pw(x)); ffn2(x)."""

    def __init__(self, f, p, k_conv, dev):
        lin = lambda q: Lin(f[q + "weight"], f[q + "bias"], dev)
        self.f1a, self.f1b, self.pw, self.f2a, self.f2b = lin(p + "ffn1.0."), lin(p + "ffn1.2."), lin(p + "pw."), lin(p + "ffn2.0."), lin(p + "ffn2.2.")
        self.dw = []
        for i, k in enumerate(k_conv):
            w, b = f[p + f"conv_list.{i}.weight"], f[p + f"conv_list.{i}.bias"]
            c = up64(w.shape[0])
            self.dw.append((pad_to(w.reshape(w.shape[0], k * k).t(), 1, c).to(H16).contiguous().to(dev), pad_to(b, 0, c).to(H16).contiguous().to(dev), k))


class MemFlowEngine(FlowEngine):
    """MemFlowNet (things_memflownet: basicencoder cnet/fnet, GMA-SK2 update block) + InferenceCore + MemoryManager
    (MemFlow.py:21-183, sk2.py, inference/inference_core_skflow.py:20-54, memory_manager_skflow.py) on the device: f16 NHWC activations
    with channel counts padded to multiples of 64, f32 coordinates / flow / correlation inputs.  `splitkv`: the key chunks asked of the memory-read
    attention (hostlogic.memflow_splitkv_chunks; below 2 = the one-pass kernel; profiles/r6_ab_memflow_splitkv.txt)."""

    def __init__(self, state_dict, device, iters=15, train_avg_length=(400 * 720 // 64) * 3 / 2, max_mt=2, min_mt=1, splitkv=3):
        missing = [k for k in memflow_param_shapes() if k not in state_dict]
        if missing:
            raise KeyError(f"MemFlowNet state dict lacks {len(missing)} keys, e.g. {missing[:3]}")
        super().__init__(device)
        self.iters, self.tal, self.max_mt, self.min_mt, self.splitkv = iters, train_avg_length, max_mt, min_mt, splitkv
        f = {k: v.float() for k, v in state_dict.items() if v.dtype.is_floating_point}
        d = self.dev
        self.fnet = EncoderEngine(state_dict, "fnet.", "instance", d)
        self.cnet = EncoderEngine(state_dict, "cnet.", "batch", d)
        u = "update_block."
        self.convc1, self.convc2 = _PCBlock(f, u + "encoder.convc1.", K_CONV, d), _PCBlock(f, u + "encoder.convc2.", K_CONV, d)
        self.convf1 = Lin(f[u + "encoder.convf1.weight"], f[u + "encoder.convf1.bias"], d)
        self.convf2, self.conv = _PCBlock(f, u + "encoder.convf2.", K_CONV, d), _PCBlock(f, u + "encoder.conv.", K_CONV, d)
        self.gru, self.flow_head = _PCBlock(f, u + "gru.", K_GRU, d), _PCBlock(f, u + "flow_head.", K_CONV, d)
        self.mask0 = self._conv3w(f[u + "mask.0.weight"], f[u + "mask.0.bias"], 256)
        self.mask2 = Lin(f[u + "mask.2.weight"], f[u + "mask.2.bias"], d)
        self.to_v = Lin(f[u + "aggregator.to_v.weight"], None, d)
        self.gamma = float(f[u + "aggregator.gamma"].item())
        self.to_qk = Lin(f["att.to_qk.weight"], None, d)
        self.scale = 128 ** -0.5                                   # Attention.scale, gma.py:47
        self.clear_memory()

    def clear_memory(self):
        self.mem_k = self.mem_v = None                             # rows [T, 128] f16 (working memory, oldest first)

    # ---- building blocks
    def _pc(self, blk, x, B, h, w, out_act=0):
        M = B * h * w
        t = self._gemm(x, blk.f1a, M, act=4)
        x = self._gemm(t, blk.f1b, M, act=5, resid=x)
        for wd, bd, k in blk.dw:
            y = torch.empty_like(x)
            self.L.tcl_dwconv_gelu_f16(x, wd, bd, y, B, h, w, x.shape[1], k, stream())
            x = y
        x = self._gemm(x, blk.pw, M, act=5, resid=x)
        t = self._gemm(x, blk.f2a, M, act=4)
        return self._gemm(t, blk.f2b, M, act=out_act)

    def _cat(self, a, b, M):
        y = torch.empty(M, a.shape[1] + b.shape[1], dtype=H16, device=self.dev)
        self.L.tcl_concat_channels_f16(a, a.shape[1], b, b.shape[1], y, M, stream())
        return y

    @torch.no_grad()
    def step(self, images, end=False, flow_init=None):
        """InferenceCore.step: images [1,2,3,H,W] f32 in [-1,1] (H, W multiples of 8; H/8/8 >= 2) -> (flow_low [1,2,H/8,W/8], flow_up [1,2,H,W]).

        A pair is kernel time, not launch gaps; replaying the step as a HIP graph was measured and lost (profiles/r6_ab_memflow_graph_nw.txt)."""
        images = images.to(self.dev).float().contiguous()
        fi = None if flow_init is None else flow_init.to(self.dev).float().contiguous()
        Tm = 0 if self.mem_k is None else self.mem_k.shape[0]
        flow_low, up, k_all, v_all = self._core(images, self.mem_k, self.mem_v, fi)
        self._remember(k_all, v_all, end, Tm)
        return flow_low, up

    def _remember(self, k_all, v_all, end, Tm):
        if not end:                                                # mem_every = 1 (inference_core_skflow.py:25, :49-51)
            self.mem_k, self.mem_v = k_all, v_all
            P = k_all.shape[0] - Tm
            if self.mem_k.shape[0] >= self.max_mt * P:             # compress_features: keep the last min_mt frames
                self.mem_k, self.mem_v = self.mem_k[-self.min_mt * P:].contiguous(), self.mem_v[-self.min_mt * P:].contiguous()

    def _core(self, images, mem_k, mem_v, flow_init):
        """The device work of one step: (images, working memory, warm start) -> (flow_low, flow_up, k_all, v_all)."""
        L, d = self.L, self.dev
        # context: net = tanh(c[:, :128]), inp = relu(c[:, 128:]), (query, key) = to_qk(inp)   (MemFlow.py:112-118)
        c, (h, w) = self.cnet.forward(images[:, 0])
        P = h * w
        net, inp = self._context_split(c, P)
        qk = self._gemm(inp, self.to_qk, P)                        # [P, 256]: query | key
        key = qk[:, 128:].contiguous()
        fm, _ = self.fnet.forward(images[0])
        fm = fm.float().view(2, h, w, 256)
        corr_fn = CorrBlock.from_nhwc(fm[0:1].contiguous(), fm[1:2].contiguous())
        coords0 = self.coords_grid(1, h, w)
        coords1 = coords0.clone() if flow_init is None else (coords0 + flow_init).contiguous()
        corr_rows = torch.zeros(P, 384, dtype=H16, device=d)       # 324 channels + zero padding
        k_all = key if mem_k is None else torch.cat([mem_k, key])
        T = k_all.shape[0]
        scale = self.scale * np.log(T) / np.log(self.tal)          # memory_manager_skflow.py:59 (math.log(T, train_avg_length))
        # one head and one entry leave the flash kernel 114 blocks at 1280x720 -- the keys are cut into chunks that run as batch entries
        # (tcl_attention_splitkv_f16)
        ns = memflow_splitkv_chunks(P, T, self.splitkv)
        if ns:
            wsp = torch.empty(L.tcl_attention_splitkv_workspace_bytes(ns, 1, P, T, 128), dtype=torch.uint8, device=d)
        else:
            wq = torch.empty(L.tcl_attention_q_bytes(1, 1, P, 128), dtype=torch.uint8, device=d)
            wkv = torch.empty(L.tcl_attention_kv_bytes(1, 1, T, 128), dtype=torch.uint8, device=d)
        for it in range(self.iters):
            corr_fn.lookup_rows(coords1, corr_rows)
            flow = coords1 - coords0
            cor = self._pc(self.convc2, self._pc(self.convc1, corr_rows, 1, h, w, out_act=4), 1, h, w)
            frow = torch.empty(P, 64, dtype=H16, device=d)
            L.tcl_nchw_f32_to_rows_f16(flow, frow, 1, 2, P, 64, 0, 1, stream())
            flo = self._pc(self.convf2, self._gemm(frow, self.convf1, P), 1, h, w)
            mf = self._pc(self.conv, self._cat(cor, flo, P), 1, h, w)          # [P,128]: 126 channels + 2 zero
            L.tcl_nchw_f32_to_rows_f16(flow, mf, 1, 2, P, 128, 126, 0, stream())  # torch.cat([out, flow], 1)   (sk2.py:128)
            val = self._gemm(mf, self.to_v, P)
            v_all = val if mem_v is None else torch.cat([mem_v, val])
            ro = torch.empty(P, 128, dtype=H16, device=d)
            if ns:
                L.tcl_attention_splitkv_f16(qk, 256, k_all, 128, v_all, 128, ro, 128, 1, P, T, 128, float(scale), ns, wsp, stream())
            else:
                L.tcl_attention_f16(qk, 256, P * 256, k_all, 128, T * 128, v_all, 128, T * 128, ro, 128, P * 128, 1, 1, P, T, 128, float(scale), 1, 1, wq, wkv,
                                    stream())
            mfg = torch.empty_like(mf)
            L.tcl_axpy_f16(mf, ro, self.gamma, mfg, mf.numel(), stream())
            net = self._pc(self.gru, self._cat(self._cat(net, inp, P), self._cat(mf, mfg, P), P), 1, h, w)
            delta = self._pc(self.flow_head, net, 1, h, w)          # [P,64]: 2 channels + zero padding
            L.tcl_rows_f16_to_nchw_f32(delta, coords1, 1, 2, P, 64, 0, 1.0, 1.0, stream())
        return (*self._upsample(net, coords0, coords1, 1, h, w), k_all, v_all)


# ------------------------------------------------------------------------------------------------ video-level driver
def forward_interpolate(flow):
    """core/utils/utils.py:32-63 (host, scipy): push every flow vector to where it points and fill by nearest neighbour -- the warm
    start of the next frame pair (video_dataparser.py:154).  flow [2,h,w] tensor -> [2,h,w] f32 CPU tensor."""
    from scipy import interpolate
    f = flow.detach().float().cpu().numpy()
    dx, dy = f[0], f[1]
    ht, wd = dx.shape
    x0, y0 = np.meshgrid(np.arange(wd), np.arange(ht))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    dxr, dyr = dx.reshape(-1), dy.reshape(-1)
    valid = (x1 > 0) & (x1 < wd) & (y1 > 0) & (y1 < ht)
    x1, y1, dxr, dyr = x1[valid], y1[valid], dxr[valid], dyr[valid]
    if len(x1) == 0:
        return torch.zeros(f.shape)
    fx = interpolate.griddata((x1, y1), dxr, (x0, y0), method="nearest", fill_value=0)
    fy = interpolate.griddata((x1, y1), dyr, (x0, y0), method="nearest", fill_value=0)
    return torch.from_numpy(np.stack([fx, fy], axis=0)).float()


def estimate_flows(engine, frames, warm_start=True):
    """VideoDataParser.load_flow / calc_flow for the 'memflow' model (video_dataparser.py:63-110, 141-156): frames [N,3,H,W] in [0,1] ->
    (future_flows, past_flows) [N,2,H,W] f32 on the device.  As in the reference ONE inference core (one working memory) serves the
    interleaved forward and backward pairs, each direction with its own warm-start chain; the last future flow and the first past flow
    are zero."""
    gts = frames.float() * 2.0 - 1.0
    N = gts.shape[0]
    fut, past = [], []
    prev = {True: None, False: None}
    engine.clear_memory()
    for idx in range(N):
        for is_future in (True, False):
            zero_idx = N - 1 if is_future else 0
            if idx == zero_idx:
                flow = torch.zeros_like(gts[idx:idx + 1, :2])
            else:
                src, tgt = gts[idx:idx + 1], (gts[idx + 1:idx + 2] if is_future else gts[idx - 1:idx])
                (src, pad), (tgt, _) = pad8(src), pad8(tgt)
                low, up = engine.step(torch.cat([src, tgt])[None], flow_init=prev[is_future] if warm_start else None)
                ht, wd = up.shape[-2:]
                flow = up[..., pad[2]:ht - pad[3], pad[0]:wd - pad[1]]
                prev[is_future] = forward_interpolate(low[0])[None].to(up.device)
            (fut if is_future else past).append(flow)
    return torch.cat(fut), torch.cat(past)
