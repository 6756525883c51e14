"""IC-Light / SD-1.5 UNet forward on the HIP C ABI, with VidToMe token merging in every transformer block.

Host-side mirror of what the reference assembles from diffusers + monkey-patching:
  UNet2DConditionModel.forward (diffusers 0.32.1; call site generate.py:342-347), the 8-channel conv_in and the
  concat_conds hook (utils/model_utils.py:21-40), ToMeBlock.forward (utils/VidToMe/vidtome/patch.py:124-201).
Activations are NHWC f16 [B, H*W, C]; every op below is one C-ABI call (tc_light_amd/csrc/*.hip).  Python only
sequences launches and owns buffers; there is no torch arithmetic on the data path.
"""
import os
from typing import NamedTuple

import torch

from .lib import TCL_ATTN_PACK_KV, TCL_ATTN_PAIR, TCL_ATTN_PREPACKED, lib, stream
from . import sd15
from .vidtome import VidToMe

H16 = torch.float16


def _dev(t, dev):
    return t.to(device=dev, dtype=H16).contiguous()


def _geglu_rows(w):
    """ff.net.0.proj rows [value (D) | gate (D)] -> 64-row groups [32 value | 32 matching gate] for the fused GEGLU epilogue."""
    D = w.shape[0] // 2
    idx = torch.arange(D).reshape(-1, 32)
    return w[torch.cat([idx, idx + D], dim=1).reshape(-1)]


def _conv_w(w, dev):          # [Cout,Cin,3,3] -> [Cout, 9*Cin] tap-major
    return _dev(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), dev)


class Switches(NamedTuple):
    """The A/B switches of the UNet pass: every fused route below can be turned off to fall back to the general one it replaced (which the shapes
    the fused kernels do not cover take anyway).  `forward_many` reads them once per pass and hands the record down."""
    gn_concat: bool       # a ResNet block's norm1 also writes the raw [x | skip] concat its 1x1 shortcut reads (else: a concat pass)
    ln_metric: bool       # norm1 of a merging block also writes VidToMe's matching metric y / |y| (else: the merge normalises the rows itself)
    qkv_panel: bool       # attn1's QKV GEMM writes the attention panels itself, d = 40 / 80 (else: a [rows, 3C] tensor and a pack launch)
    merge_lazy: bool      # ... and gathers the merged sequence in its operand load (else: the merge materialises it)
    ln_gemm: bool         # C = 320: norm2 / norm3 ride in the operand load of to_q / the GEGLU Linear (else: a LayerNorm pass each)
    qpanel: bool          # ... and norm2 -> to_q writes attn2's query panel directly, once the text K/V are packed (else: an [M, C] q and a pack pass)
    tome_stream: bool     # the matching chain of the merging blocks runs on a side stream, ahead of the attention (else: in line on the main stream)
    cfg_dedup: bool       # forward_many(cfg_pair=True) computes the text-free prefix of the two guidance halves once (else: both halves)

    @classmethod
    def from_env(cls):
        """TCL_GN_CONCAT, TCL_LN_METRIC, TCL_QKV_PANEL, TCL_MERGE_LAZY, TCL_LN_GEMM, TCL_QPANEL, TCL_TOME_STREAM, TCL_CFG_DEDUP (TCL_ + the field's
        name): on unless the variable is "0"."""
        return cls(*(os.environ.get("TCL_" + f.upper(), "1") != "0" for f in cls._fields))


class FrameText:
    """generation.prompt_path: a text conditioning per frame instead of one per guidance half.  neg [L, 768] f16 is the negative prompt all frames
    share, rows [R, L, 768] f16 the distinct per-frame embeddings (tcl_text_lerp_f16) and index[f] the row of LOCAL frame f.  `text` [1 + R, L, 768]
    is what every transformer block projects to K | V once per run: entry 0 the negative, entry 1 + r row r."""

    def __init__(self, neg, rows, index):
        R, Lt, D = rows.shape
        if tuple(neg.shape[-2:]) != (Lt, D) or neg.numel() != Lt * D:
            raise ValueError(f"FrameText: negative embedding {tuple(neg.shape)} against rows {tuple(rows.shape)}")
        self.index = [int(i) for i in index]
        if not self.index or min(self.index) < 0 or max(self.index) >= R:
            raise ValueError(f"FrameText: frame -> row table outside [0, {R})")
        self.rows = R
        self.text = torch.cat([neg.reshape(1, Lt, D).to(rows), rows]).to(H16).contiguous()

    def kv_index(self, frames, dev):
        """The K / V entry of every sample of a pass over `frames` (local ids, in sample order): the unconditional half takes entry 0, the conditional
        sample of frame f entry 1 + index[f].  -> KVIndex, built on the host and uploaded once per pass."""
        host = torch.tensor([0] * len(frames) + [1 + self.index[f] for f in frames], dtype=torch.int32)
        return KVIndex(host.to(dev), host, 1 + self.rows)


class KVIndex(NamedTuple):
    dev: torch.Tensor      # int32 [B] on the device
    host: torch.Tensor     # the same table on the host: tcl_attention_kvindex_f16 checks its range there
    rows: int              # entries of the K / V panels


class ImagePrompt:
    """generation.ip_adapter: the image conditioning of IP-Adapter (decoupled cross-attention beside every text cross-attention).  tokens [2, Tip, 768]
    f16: entry 0 the tokens of the zero image embedding (the unconditional half), entry 1 those of the reference image; weights {transformer block
    prefix: [2C, 768] f16 = to_k_ip ; to_v_ip of that block}; scale in [0, 2].  Every block projects the tokens to K_ip | V_ip once per run
    (UNetEngine._ip_kv); `tcl_attention_ip_add_f16` then adds scale * softmax(q K_ip^T) V_ip to the text attention's output."""

    def __init__(self, tokens, weights, scale):
        if tokens.dim() != 3 or tokens.shape[0] != 2 or not 1 <= tokens.shape[1] <= 16 or tokens.dtype != H16:
            raise ValueError(f"ImagePrompt: tokens {tuple(tokens.shape)} {tokens.dtype}, expected [2, 1..16, D] f16 (zero image, reference image)")
        self.tokens, self.weights, self.scale = tokens.contiguous(), weights, float(scale)
        self.n_tokens = int(tokens.shape[1])


class _IpCall(NamedTuple):
    kv: torch.Tensor       # [2, Tip, 2C] f16: K_ip | V_ip of this block, entry 0 the zero image's
    n_tokens: int
    scale: float


GEMM_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tune_gfx950.txt")


def load_gemm_table(L):
    """The committed GEMM tile table (shape -> tile configuration, measured on an MI355X by `bench.py --save_gemm_table`): loaded once per
    process, so known shapes never pay the in-call autotuner (no host sync in the hot loop, same tile run to run).  TCL_GEMM_TABLE overrides
    the path; TCL_AUTOTUNE = 1 (default: time shapes the table lacks on first use), "table" (never time: static heuristic for missing
    shapes) or 0 (static heuristic only).  Results are bit-identical whatever tile is chosen (tests/test_gpu_kernels.py)."""
    if getattr(load_gemm_table, "done", False):
        return
    load_gemm_table.done = True
    mode = os.environ.get("TCL_AUTOTUNE", "1")
    if mode == "0":
        L.tcl_gemm_autotune(0)
        return
    path = os.environ.get("TCL_GEMM_TABLE", GEMM_TABLE)
    if os.path.exists(path):
        try:                    # (the ctypes binding raises on a non-zero return code: an unversioned / foreign table is TCL_EINVAL)
            L.tcl_gemm_tune_load(path)
        except RuntimeError:
            import warnings
            warnings.warn(f"GEMM tile table {path} was written for other kernels (no / other version line): ignored, shapes are timed on first use")
    L.tcl_gemm_autotune(2 if mode == "table" else 1)


class Ops:
    """Thin typed wrappers around the C ABI (allocation via torch's caching allocator, launches on the current stream)."""
    _splitk_ws = {}

    def __init__(self, dev):
        self.dev = dev
        self.L = lib()
        load_gemm_table(self.L)
        self._gn_ws = {}
        ws = Ops._splitk_ws.get(str(dev))
        if ws is None:      # one split-K scratch per device, registered with the library (single compute stream)
            ws = Ops._splitk_ws[str(dev)] = torch.empty(96 << 20, dtype=torch.uint8, device=dev)
            self.L.tcl_set_workspace(ws, ws.numel())

    def empty(self, *shape, dtype=H16):
        return torch.empty(*shape, dtype=dtype, device=self.dev)

    def gemm(self, a, w, bias=None, resid=None, act=0, out=None, M=None, lda=None, N=None, K=None, ldw=None, ldc=None):
        if N is None:
            N, K = w.shape
        M = M if M is not None else a.numel() // K
        No = N // 2 if act == 2 else N                      # act 2 = fused GEGLU: output is [M, N/2]
        c = out if out is not None else self.empty(M, No)
        self.L.tcl_gemm_f16(a, w, bias if bias is not None else 0, resid if resid is not None else 0, c, M, N, K,
                            lda or K, ldw or K, ldc or No, N, act, stream())
        return c

    def conv3x3(self, x, B, Hh, Ww, cin, w, bias, resid=None, stride=1, pad=1, up=None):
        cout = w.shape[0]
        Hu, Wu = up if up else (Hh, Ww)
        Ho = (Hu + 2 - 3) // stride + 1 if pad else (Hu + 1 - 3) // stride + 1
        Wo = (Wu + 2 - 3) // stride + 1 if pad else (Wu + 1 - 3) // stride + 1
        y = self.empty(B * Ho * Wo, cout)
        self.L.tcl_conv3x3_f16(x, w, bias if bias is not None else 0, resid if resid is not None else 0, y, B, Hh, Ww, cin, cout,
                               stride, pad, up[0] if up else 0, up[1] if up else 0, 0, stream())
        return y, Ho, Wo

    def groupnorm(self, x1, c1, gamma, beta, B, HW, eps, silu, x2=None, c2=0, groups=32, raw=False):
        """raw=True: also return the un-normalised concat [x1 | x2] (written by the same pass) -> (y, yraw)."""
        key = (B, c1 + c2)
        ws = self._gn_ws.get(key)
        if ws is None:
            ws = self._gn_ws[key] = torch.zeros(self.L.tcl_groupnorm_workspace_bytes(B, c1 + c2), dtype=torch.uint8, device=self.dev)   # zeroed once
        y = self.empty(B * HW, c1 + c2)
        if raw:
            yr = self.empty(B * HW, c1 + c2)
            self.L.tcl_groupnorm_concat_f16(x1, c1, x2 if x2 is not None else 0, c2, gamma, beta, y, yr, B, HW, groups, eps, int(silu), ws, stream())
            return y, yr
        self.L.tcl_groupnorm_f16(x1, c1, x2 if x2 is not None else 0, c2, gamma, beta, y, B, HW, groups, eps, int(silu), ws, stream())
        return y

    def layernorm(self, x, gamma, beta, rows, C, metric=False):
        y = self.empty(rows, C)
        if metric:          # norm1 of a VidToMe-patched block: the matching metric y / |y| leaves the same kernel
            m = self.empty(rows, C)
            self.L.tcl_layernorm_metric_f16(x, gamma, beta, y, m, rows, C, 1e-5, stream())
            return y, m
        self.L.tcl_layernorm_f16(x, gamma, beta, y, rows, C, 1e-5, stream())
        return y

    def ln_gemm(self, x, gamma, beta, w, bias=None, act=0):
        """act(LayerNorm(x) @ w.T + bias) in one kernel (K = 320: csrc/linstrip.hip); the normalised activations are never written."""
        N, K = w.shape
        M = x.numel() // K
        c = self.empty(M, N // 2 if act == 2 else N)
        self.L.tcl_ln_gemm_f16(x, gamma, beta, 1e-5, w, bias if bias is not None else 0, 0, c, M, N, K, K, K, c.shape[1], N, act, stream())
        return c

    def attention(self, q, ldq, qbs, k, ldk, kbs, v, ldv, vbs, B, Hh, Tq, Tk, d, kv_div=1, ws_kv=None, pack_kv=True, pair=False, kvi=None):
        """Strided operands: Q is packed into a fresh panel workspace, K / V into ws_kv (pack_kv=False: ws_kv already holds them packed).
        kvi (KVIndex): every sample's K / V entry comes from that table instead of b // kv_div; ws_kv holds kvi.rows entries."""
        o = self.empty(B * Tq, Hh * d)
        wq = torch.empty(self.L.tcl_attention_q_bytes(B, Hh, Tq, d), dtype=torch.uint8, device=self.dev)
        if kvi is not None:
            self.L.tcl_attention_kvindex_f16(q, ldq, qbs, k, ldk, kbs, v, ldv, vbs, o, Hh * d, Tq * Hh * d, B, Hh, Tq, Tk, d, d ** -0.5, 1,
                                             (TCL_ATTN_PACK_KV if pack_kv else 0) | (TCL_ATTN_PAIR if pair else 0), wq, ws_kv, kvi.dev, kvi.host, kvi.rows,
                                             stream())
            return o
        if ws_kv is None:
            ws_kv = torch.empty(self.L.tcl_attention_kv_bytes(B // kv_div, Hh, Tk, d), dtype=torch.uint8, device=self.dev)
        self.L.tcl_attention_f16(q, ldq, qbs, k, ldk, kbs, v, ldv, vbs, o, Hh * d, Tq * Hh * d, B, Hh, Tq, Tk, d, d ** -0.5, kv_div,
                                 (TCL_ATTN_PACK_KV if pack_kv else 0) | (TCL_ATTN_PAIR if pair else 0), wq, ws_kv, stream())
        return o

    def attention_prepacked(self, wq, wkv, B, Hh, Tq, Tk, d, kv_div=1, pair=False, ldq=0, qbs=0, kvi=None):
        """Panels already filled by tcl_gemm_qkv_panels_f16 / tcl_ln_gemm_qpanel_f16; ldq / qbs: strides of the Q tensor never written (the ABI takes them)."""
        o = self.empty(B * Tq, Hh * d)
        if kvi is not None:
            self.L.tcl_attention_kvindex_f16(wq, ldq, qbs, 0, 0, 0, 0, 0, 0, o, Hh * d, Tq * Hh * d, B, Hh, Tq, Tk, d, d ** -0.5, 1,
                                             TCL_ATTN_PREPACKED | (TCL_ATTN_PAIR if pair else 0), wq, wkv, kvi.dev, kvi.host, kvi.rows, stream())
            return o
        self.L.tcl_attention_f16(wq, ldq, qbs, 0, 0, 0, 0, 0, 0, o, Hh * d, Tq * Hh * d, B, Hh, Tq, Tk, d, d ** -0.5, kv_div,
                                 TCL_ATTN_PREPACKED | (TCL_ATTN_PAIR if pair else 0), wq, wkv, stream())
        return o


class UNetEngine:
    """unet(sample[2F,4,h',w'], t, encoder_hidden_states=[2F,L,768], cross_attention_kwargs={'concat_conds': ...}).sample
    is served by `forward_nhwc` (NHWC in/out) so that the pack/unpack kernels can feed it without layout round trips."""

    in_channels = 4   # unet.config.in_channels stays 4 (generate.py:174)

    def __init__(self, state_dict, device, vidtome=None):
        self.dev = torch.device(device)
        self.ops = Ops(self.dev)
        self.L = lib()
        self.tome = vidtome if vidtome is not None else VidToMe(self.dev)
        sd = state_dict
        exp = sd15.unet_param_shapes()
        missing = [k for k in exp if k not in sd]
        if missing:
            raise KeyError(f"UNet state dict lacks {len(missing)} keys, e.g. {missing[:3]}")
        d = self.dev
        w = {}
        ci = sd["conv_in.weight"]
        wi = torch.zeros(320, 128)
        wi[:, :9 * ci.shape[1]] = ci.permute(0, 2, 3, 1).reshape(320, -1)
        w["conv_in"] = (_dev(wi, d), _dev(sd["conv_in.bias"], d), ci.shape[1])
        w["t1"] = (_dev(sd["time_embedding.linear_1.weight"], d), _dev(sd["time_embedding.linear_1.bias"], d))
        w["t2"] = (_dev(sd["time_embedding.linear_2.weight"], d), _dev(sd["time_embedding.linear_2.bias"], d))
        self.res, self.tfm = {}, {}
        for k in exp:
            if k.endswith("norm1.weight") and ".resnets." in k:
                self.res[k[:-len("norm1.weight")]] = None
            if k.endswith("proj_in.weight"):
                self.tfm[k[:-len("proj_in.weight")]] = None
        for p in self.res:
            r = dict(n1=(_dev(sd[p + "norm1.weight"], d), _dev(sd[p + "norm1.bias"], d)),
                     c1=_conv_w(sd[p + "conv1.weight"], d), b1=_dev(sd[p + "conv1.bias"], d),
                     tw=_dev(sd[p + "time_emb_proj.weight"], d), tb=_dev(sd[p + "time_emb_proj.bias"], d),
                     n2=(_dev(sd[p + "norm2.weight"], d), _dev(sd[p + "norm2.bias"], d)),
                     c2=_conv_w(sd[p + "conv2.weight"], d), b2=_dev(sd[p + "conv2.bias"], d),
                     cin=sd[p + "conv1.weight"].shape[1], cout=sd[p + "conv1.weight"].shape[0])
            if p + "conv_shortcut.weight" in sd:
                r["sc"] = (_dev(sd[p + "conv_shortcut.weight"].flatten(1), d), _dev(sd[p + "conv_shortcut.bias"], d))
            self.res[p] = r
        for p in self.tfm:
            t = p + "transformer_blocks.0."
            c = sd[p + "proj_in.weight"].shape[0]
            self.tfm[p] = dict(
                c=c, gn=(_dev(sd[p + "norm.weight"], d), _dev(sd[p + "norm.bias"], d)),
                pin=(_dev(sd[p + "proj_in.weight"].flatten(1), d), _dev(sd[p + "proj_in.bias"], d)),
                pout=(_dev(sd[p + "proj_out.weight"].flatten(1), d), _dev(sd[p + "proj_out.bias"], d)),
                ln=[(_dev(sd[t + f"norm{i}.weight"], d), _dev(sd[t + f"norm{i}.bias"], d)) for i in (1, 2, 3)],
                qkv=_dev(torch.cat([sd[t + "attn1.to_q.weight"], sd[t + "attn1.to_k.weight"], sd[t + "attn1.to_v.weight"]]), d),
                o1=(_dev(sd[t + "attn1.to_out.0.weight"], d), _dev(sd[t + "attn1.to_out.0.bias"], d)),
                q2=_dev(sd[t + "attn2.to_q.weight"], d),
                kv2=_dev(torch.cat([sd[t + "attn2.to_k.weight"], sd[t + "attn2.to_v.weight"]]), d),
                o2=(_dev(sd[t + "attn2.to_out.0.weight"], d), _dev(sd[t + "attn2.to_out.0.bias"], d)),
                ff1=(_dev(_geglu_rows(sd[t + "ff.net.0.proj.weight"]), d), _dev(_geglu_rows(sd[t + "ff.net.0.proj.bias"]), d)),
                ff2=(_dev(sd[t + "ff.net.2.weight"], d), _dev(sd[t + "ff.net.2.bias"], d)),
                text_kv={}, ip_kv=None)
        for i in range(3):
            w[f"down{i}"] = (_conv_w(sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], d), _dev(sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], d))
            w[f"up{i}"] = (_conv_w(sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], d), _dev(sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], d))
        w["norm_out"] = (_dev(sd["conv_norm_out.weight"], d), _dev(sd["conv_norm_out.bias"], d))
        w["conv_out"] = (_conv_w(sd["conv_out.weight"], d), _dev(sd["conv_out.bias"], d))
        self.w = w
        self._temb_cache = (None, None)
        self._panel_cache, self._qpanels = {}, {}    # attn1's (Q, K / V^T) panels (`_attn_panels`, at most _panel_cap bytes), attn2's Q panels (`_q_panel`)
        self._panel_cap = self._side = None          # set on first use: `panel_cache_cap`; the matching chain's stream (`_attn1_merged`)
        self.flops = 0.0          # algorithmic FLOPs (2*MACs) of the reference's computation, accumulated per forward for the roofline figure
        self.flops_executed = 0.0  # FLOPs that actually ran (== flops without the CFG-pair de-duplication)
        self.count_flops = False

    # ------------------------------------------------------------------ time embedding (once per timestep)
    def _temb(self, t):
        t = float(t)
        if self._temb_cache[0] == t:
            return self._temb_cache[1]
        o, L = self.ops, self.L
        e0 = o.empty(320); L.tcl_timestep_embed_f16(t, 320, e0, stream())
        e1 = o.empty(1280); L.tcl_gemv_f16(self.w["t1"][0], e0, self.w["t1"][1], 0, e1, 1280, 320, 0, 1, stream())
        emb = o.empty(1280); L.tcl_gemv_f16(self.w["t2"][0], e1, self.w["t2"][1], 0, emb, 1280, 1280, 0, 0, stream())
        proj = {}
        for p, r in self.res.items():   # conv1 bias + time_emb_proj(silu(emb)) folded into one per-channel vector
            v = o.empty(r["cout"])
            L.tcl_gemv_f16(r["tw"], emb, r["tb"], r["b1"], v, r["cout"], 1280, 1, 0, stream())
            proj[p] = v
        self._temb_cache = (t, proj)
        return proj

    # ------------------------------------------------------------------ blocks
    def _resblock(self, p, x, B, Hh, Ww, tproj, sw, skip=None, cskip=0, rep=1):
        """rep: how many identical copies of these B samples the reference computes (FLOP accounting only)."""
        o, r = self.ops, self.res[p]
        HW = Hh * Ww
        cx = r["cin"] - cskip
        fuse_cat = skip is not None and "sc" in r and sw.gn_concat
        hn = o.groupnorm(x, cx, *r["n1"], B, HW, 1e-5, True, x2=skip, c2=cskip, raw=fuse_cat)
        if fuse_cat:            # norm1's apply pass reads x and skip anyway: it writes the raw concat for the 1x1 shortcut as well (same bits as a concat pass)
            hn, xc = hn
        h1, _, _ = o.conv3x3(hn, B, Hh, Ww, r["cin"], r["c1"], tproj[p])
        hn2 = o.groupnorm(h1, r["cout"], *r["n2"], B, HW, 1e-5, True)
        if "sc" in r:
            if skip is None:
                xc = x
            elif not fuse_cat:
                xc = o.empty(B * HW, r["cin"])
                self.L.tcl_concat_channels_f16(x, cx, skip, cskip, xc, B * HW, stream())
            xs = o.gemm(xc, r["sc"][0], r["sc"][1])
            self._fl(2.0 * HW * r["cin"] * r["cout"], rep * B, B)
        else:
            xs = x
        out, _, _ = o.conv3x3(hn2, B, Hh, Ww, r["cout"], r["c2"], r["b2"], resid=xs)
        self._fl(2.0 * HW * 9 * (r["cin"] + r["cout"]) * r["cout"], rep * B, B)
        return out

    def _fl(self, f, n=1, n_executed=None):
        """f FLOPs per sample / row: n of them in the reference's computation, n_executed run here (fewer where the CFG halves run once); exact integers."""
        if self.count_flops:
            self.flops += f * n
            self.flops_executed += f * (n if n_executed is None else n_executed)

    def _text_kv(self, blk, text):
        key = id(text)
        hit = blk["text_kv"].get(key)
        if hit is None:
            o = self.ops
            Bt, Lt, _ = text.shape
            c = blk["c"]
            kv = o.gemm(text, blk["kv2"])                        # [Bt*L, 2C]: K | V
            ws = torch.empty(self.L.tcl_attention_kv_bytes(Bt, sd15.HEADS, Lt, c // sd15.HEADS), dtype=torch.uint8, device=self.dev)
            hit = blk["text_kv"][key] = dict(kv=kv, ws=ws, packed=False, L=Lt, text=text)
        return hit

    def _ip_kv(self, p, blk, ip):
        """K_ip | V_ip of block `p` for the ImagePrompt `ip`: tokens @ [to_k_ip ; to_v_ip]^T -> [2, Tip, 2C] f16, one GEMM per block and run (the last
        ImagePrompt's projection is kept beside the text K / V)."""
        if ip is None:
            return None
        hit = blk["ip_kv"]
        if hit is None or hit[0] is not ip:
            w = ip.weights.get(p)
            if w is None or tuple(w.shape) != (2 * blk["c"], ip.tokens.shape[2]):
                raise ValueError(f"ImagePrompt: block {p} needs [to_k_ip ; to_v_ip] of shape {(2 * blk['c'], ip.tokens.shape[2])}, got "
                                 f"{None if w is None else tuple(w.shape)}")
            hit = blk["ip_kv"] = (ip, self.ops.gemm(ip.tokens, w))
        return _IpCall(hit[1], ip.n_tokens, ip.scale)

    def _q_panel(self, B, Hh, Tq, d):
        """A zero-initialised query-panel workspace per shape, reused by every block (stream order serialises them): tcl_ln_gemm_qpanel_f16 writes the
        rows t < Tq of every (sample, head) panel and never touches the padding rows, which therefore stay zero."""
        key = (B, Hh, Tq, d)
        cache = self._qpanels
        if key not in cache:
            if len(cache) > 4:
                cache.clear()
            cache[key] = torch.zeros(self.L.tcl_attention_q_bytes(B, Hh, Tq, d), dtype=torch.uint8, device=self.dev)
        return cache[key]

    def panel_cache_cap(self):
        """Byte bound of the persistent attention-panel cache: 8 % of the device's memory, at most 24 GiB; Generator.__init__'s token budget subtracts it."""
        if self._panel_cap is None:
            total = torch.cuda.get_device_properties(self.dev).total_memory if self.dev.type == "cuda" and torch.cuda.is_available() else (288 << 30)
            self._panel_cap = int(min(24 << 30, 0.08 * total))
        return self._panel_cap

    def panel_cache_bytes(self):
        return sum(a.numel() + b.numel() for a, b in self._panel_cache.values())

    def text_rows_bytes(self, rows, Lt=77):
        """Bytes the K / V panels of `rows` text entries hold over all transformer blocks (tcl_attention_kv_bytes per block): what a FrameText of that many
        rows keeps resident beside the pass.  Generator.__init__'s token budget subtracts it."""
        return sum(self.L.tcl_attention_kv_bytes(int(rows), sd15.HEADS, Lt, blk["c"] // sd15.HEADS) for blk in self.tfm.values())

    def drop_panels(self):
        self._panel_cache.clear()
        self._qpanels.clear()

    def _attn_panels(self, ne, Hh, T, d):
        """Zero-initialised Q and K / V^T panel workspaces per (entries, heads, merged length, head_dim), reused by every chunk and block that meets the shape
        again (all on the main stream: stream order serialises writer and readers).  tcl_gemm_qkv_panels_f16 never writes the panels' padding, which therefore
        stays zero.  The merged lengths of a clip are a handful of values (chunk lengths 1..4 x which side of the global merge is src); the cache is bounded."""
        key = (ne, Hh, T, d)
        cache = self._panel_cache
        hit = cache.pop(key, None)
        if hit is None:
            nq, nkv = self.L.tcl_attention_q_bytes(ne, Hh, T, d), self.L.tcl_attention_kv_bytes(ne, Hh, T, d)
            while cache and self.panel_cache_bytes() + nq + nkv > self.panel_cache_cap():
                cache.pop(next(iter(cache)))                      # oldest first (dict order = insertion / last use)
            try:
                hit = (torch.zeros(nq, dtype=torch.uint8, device=self.dev), torch.zeros(nkv, dtype=torch.uint8, device=self.dev))
            except torch.OutOfMemoryError:                        # a shared / smaller device: give the cached panels back and try once more
                cache.clear()
                torch.cuda.empty_cache()
                hit = (torch.zeros(nq, dtype=torch.uint8, device=self.dev), torch.zeros(nkv, dtype=torch.uint8, device=self.dev))
        cache[key] = hit
        return hit

    def _attn1_plain(self, blk, h, n1, B, N, ne):
        """attn1 of a level that does not merge (downsample > max_downsample): per-frame attention over all the samples present, in one launch."""
        o, C, Hd, Bx = self.ops, blk["c"], sd15.HEADS, B // 2 * ne
        qkv = o.gemm(n1, blk["qkv"])
        a = o.attention(qkv, 3 * C, N * 3 * C, qkv[:, C:], 3 * C, N * 3 * C, qkv[:, 2 * C:], 3 * C, N * 3 * C, Bx, Hd, N, N, C // Hd, pair=ne == 1)
        self._fl(2.0 * N * C * C * 4 + 4.0 * N * N * C, B, Bx)
        return o.gemm(a, blk["o1"][0], blk["o1"][1], resid=h)

    def _attn1_merged(self, p, blk, h, n1, m1, Fs, N, ne, sw):
        """attn1 over VidToMe-merged tokens, added into h chunk by chunk: each chunk's merge uses and updates this block's bank (patch.py:59-82, 161-179).
        The matching chain runs on a side stream, ahead of the attention of the chunks already matched (single-chunk passes too: the banks stay in its pool)."""
        C = blk["c"]
        xbs = sum(Fs) * N * C                                   # a chunk's conditional rows sit xbs elements after its unconditional ones
        qkv_panel = C // sd15.HEADS in (40, 80) and sw.qkv_panel
        main = side = torch.cuda.current_stream()
        if sw.tome_stream:
            side = self._side = self._side or torch.cuda.Stream(device=self.dev)
            side.wait_stream(main)                              # n1 is ready
        off = 0
        for ci, F in enumerate(Fs):
            self.tome.select_chunk(ci)
            with torch.cuda.stream(side):
                merged, unm, T = self.tome.compute_merge(p, n1[off * N:], F, N, C, xbs=xbs, metric=m1[off * N:] if m1 is not None else None, ne=ne,
                                                         lazy_merged=qkv_panel and sw.merge_lazy)
            if sw.tome_stream:
                main.wait_event(side.record_event())
                for tns in (merged.block, merged.index, unm):
                    if tns is not None:                         # allocated on the side stream's pool, read on the main stream
                        tns.record_stream(main)
            self._attend_chunk(blk, h[off * N:], xbs, merged, unm, T, F * N, ne, qkv_panel)
            off += F
        return h

    def _attend_chunk(self, blk, h, xbs, merged, unm, T, FN, ne, qkv_panel):
        o, C, Hd, d = self.ops, blk["c"], sd15.HEADS, blk["c"] // sd15.HEADS
        if qkv_panel:
            # the QKV GEMM writes the attention panels itself (gemm.hip QP epilogue) and gathers a lazily merged sequence in its operand load
            wq, wkv = self._attn_panels(ne, Hd, T, d)
            self.L.tcl_gemm_qkv_panels_f16(merged.block, merged.entry_stride, merged.index, blk["qkv"], ne, T, Hd, d, C, C, C, d ** -0.5, wq, wkv, stream())
            a = o.attention_prepacked(wq, wkv, ne, Hd, T, T, d, pair=ne == 1, ldq=3 * C, qbs=T * 3 * C)
        else:
            qkv = o.gemm(merged.block, blk["qkv"], M=ne * T)
            a = o.attention(qkv, 3 * C, T * 3 * C, qkv[:, C:], 3 * C, T * 3 * C, qkv[:, 2 * C:], 3 * C, T * 3 * C, ne, Hd, T, T, d, pair=ne == 1)
        y = o.gemm(a, blk["o1"][0], blk["o1"][1], M=ne * T)
        self.tome.unmerge_add(h, xbs, y, T, unm, FN, C, ne)
        self._fl(2.0 * T * C * C * 4 + 4.0 * T * T * C, 2, ne)

    def attn2(self, p, h, B, N, text, ip=None):
        """attn2 of transformer block `p` alone (h [B*N, C] f16 -> h + to_out(attention), B = the two guidance halves): the unit the block tests run."""
        sw, blk = Switches.from_env(), self.tfm[p]
        return self._attn2(blk, h, B, N, text, blk["c"] == 320 and sw.ln_gemm, sw.qpanel, ip=self._ip_kv(p, blk, ip))

    def _attn2(self, blk, h, B, N, text, fuse_ln, qpanel, kvi=None, ip=None):
        """Text cross-attention on the full tokens; every sample of a guidance half shares that half's text K / V (kv_div).
        kvi (text is a FrameText): every sample attends to the K / V of its own frame's row; the rows are projected and packed once per run, after which
        only their panels are kept.
        ip (_IpCall): the image tokens' attention is added to the text attention's output before to_out (IP-Adapter); it reads the [M, C] query, so the
        query-panel route, which leaves none, is not taken while it is set (the un-fused route writes the same panel bits)."""
        o, C, Hd, d, M = self.ops, blk["c"], sd15.HEADS, blk["c"] // sd15.HEADS, B * N
        tk = self._text_kv(blk, text.text if kvi is not None else text)
        Lt = tk["L"]
        if fuse_ln and qpanel and tk["packed"] and ip is None:
            # norm2 -> to_q straight into the attention kernel's query panel (linstrip.hip Q-panel epilogue): no [M, C] output, no pack pass
            wq = self._q_panel(B, Hd, N, d)
            self.L.tcl_ln_gemm_qpanel_f16(h, *blk["ln"][1], 1e-5, blk["q2"], M, Hd, d, N, C, C, d ** -0.5, wq, stream())
            a = o.attention_prepacked(wq, tk["ws"], B, Hd, N, Lt, d, kv_div=B // 2, ldq=C, qbs=N * C, kvi=kvi)
        else:
            q = o.ln_gemm(h, *blk["ln"][1], blk["q2"]) if fuse_ln else o.gemm(o.layernorm(h, *blk["ln"][1], M, C), blk["q2"])
            kv = tk["kv"]
            a = o.attention(q, C, N * C, kv if kv is not None else 0, 2 * C, Lt * 2 * C, kv[:, C:] if kv is not None else 0, 2 * C, Lt * 2 * C, B, Hd, N, Lt, d,
                            kv_div=B // 2, ws_kv=tk["ws"], pack_kv=not tk["packed"], kvi=kvi)
            if ip is not None:
                self.L.tcl_attention_ip_add_f16(q, C, N * C, ip.kv, a, C, N * C, B, Hd, N, ip.n_tokens, d, d ** -0.5, ip.scale, B // 2, stream())
        tk["packed"] = True
        if kvi is not None:
            tk["kv"] = None                                     # the [rows * L, 2C] projection is read by the pack alone
        self._fl(2.0 * C * C * 2 + 4.0 * Lt * C, M)
        return o.gemm(a, blk["o2"][0], blk["o2"][1], resid=h)

    def _feed_forward(self, blk, h, M, fuse_ln):
        o, C = self.ops, blk["c"]                               # Linear(C -> 8C) + GEGLU fused in the GEMM epilogue -> [M, 4C], then Linear(4C -> C)
        f2 = o.ln_gemm(h, *blk["ln"][2], *blk["ff1"], act=2) if fuse_ln else o.gemm(o.layernorm(h, *blk["ln"][2], M, C), *blk["ff1"], act=2)
        self._fl(2.0 * C * C * 12, M)
        return o.gemm(f2, blk["ff2"][0], blk["ff2"][1], resid=h)

    def _transformer(self, p, x, B, Fs, Hh, Ww, text, sw, pair_half=False, kvi=None, ip=None):
        """x [B*N, C], B = 2*sum(Fs) samples: the unconditional ones of all chunks, then the conditional ones; only `_attn1_merged` goes chunk by chunk.
        pair_half: x holds only the FIRST half of the B samples (see forward_many: the two classifier-free-guidance halves are identical up to
        the first text cross-attention); proj_in, norm1, the VidToMe merge and attn1 run on that half, the result is duplicated before attn2."""
        o, blk = self.ops, self.tfm[p]
        C, N = blk["c"], Hh * Ww
        ne = 1 if pair_half else 2                              # batch entries physically present through attn1
        Bx = B // 2 * ne
        hn = o.groupnorm(x, C, *blk["gn"], Bx, N, 1e-6, False)
        h = o.gemm(hn, blk["pin"][0], blk["pin"][1])
        self._fl(2.0 * N * C * C * 2, B, Bx)                    # proj_in and proj_out
        merging = self.tome.merges(N)
        n1, m1 = o.layernorm(h, *blk["ln"][0], Bx * N, C, metric=True) if merging and sw.ln_metric else (o.layernorm(h, *blk["ln"][0], Bx * N, C), None)
        h = self._attn1_merged(p, blk, h, n1, m1, Fs, N, ne, sw) if merging else self._attn1_plain(blk, h, n1, B, N, ne)
        if pair_half:                                           # from here on the halves differ (text): both exist
            h, x = torch.cat([h, h]), torch.cat([x, x])
        fuse_ln = C == 320 and sw.ln_gemm                       # norm2 / norm3 ride in the consumer's operand load (strip-resident Linear)
        h = self._attn2(blk, h, B, N, text, fuse_ln, sw.qpanel, kvi, self._ip_kv(p, blk, ip))
        h = self._feed_forward(blk, h, B * N, fuse_ln)
        return o.gemm(h, blk["pout"][0], blk["pout"][1], resid=x)

    # ------------------------------------------------------------------ forward
    # All chunks of a denoising step go through the UNet in ONE pass, stacked on the batch axis (unconditional samples of every
    # chunk first, then the conditional ones).  The only chunk-to-chunk dependency of the reference loop (generate.py:220-224) is
    # the global-token bank of the merging transformer blocks (levels 0 and 1; patch.py:59-82): chunk c's attn1 in block b needs
    # the bank block b was left with by chunk c-1.  Running block-major (all chunks through block b, then block b+1) keeps both
    # orders -- data flow per chunk, bank order per block -- so inside a block only attn1 loops over the chunks; ResNet blocks,
    # norms, cross-attention, feed-forward and the non-merging levels see 8-31x more rows per GEMM and one launch instead of one
    # per chunk, and every weight matrix is streamed once per step.
    def forward_many(self, x_in, Fs, Hh, Ww, t, text, cfg_pair=False, frames=None, ip=None):
        """x_in [2*Ftot, Hh, Ww, 8] f16 (latents | concat_conds; Ftot = sum(Fs) samples in chunk order, twice: uncond, cond);
        text [2, L, 768] f16 (uncond, cond).  Fs: chunk lengths in the reference's chunk order.  -> eps [2*Ftot, Hh, Ww, 4] f16.
        cfg_pair: the caller GUARANTEES x_in[Ftot:] == x_in[:Ftot] (the classifier-free-guidance pair of generate.py:342-347: `torch.cat([latents] * 2)`
        and the same concat_conds, written twice by tcl_pack_latents_f16).  The two halves then differ only through the text, which first enters in
        attn2 of the first transformer block: conv_in, the first ResNet block and proj_in / norm1 / VidToMe merge / attn1 of that block run ONCE and
        are duplicated -- the same bits as computing them twice (every kernel is deterministic and batch-row independent; with equal scores in both
        entries the matching picks the first: `test_cfg_pair_dedup_bit_identical`).  TCL_CFG_DEDUP=0 computes both halves.
        text a FrameText (generation.prompt_path): frames = the local frame id of each of the Ftot samples, in sample order; every conditional sample
        then attends to its own frame's text, the unconditional half to the one negative.  The prefix shared by the halves ends at the first attn2.
        ip (ImagePrompt; generation.ip_adapter): every attn2 also attends to the image tokens -- the unconditional half to the zero image's, the
        conditional half to the reference image's.  None: the pass is launch for launch what it was."""
        o, L, w = self.ops, self.L, self.w
        Ftot = sum(Fs)
        B = 2 * Ftot
        kvi = None
        if isinstance(text, FrameText):
            if frames is None or len(frames) != Ftot:
                raise ValueError(f"forward_many: per-frame text needs the frame id of each of the {Ftot} samples (frames=...)")
            kvi = text.kv_index([int(f) for f in frames], self.dev)      # one upload per pass, shared by the 16 blocks
        sw = Switches.from_env()                                # per pass: callers flip switches between two passes of one engine
        half = bool(cfg_pair) and sw.cfg_dedup
        Bh = Ftot if half else B                                # samples through the text-free prefix
        tproj = self._temb(t)
        self.tome.begin_step(Fs, (Hh, Ww))                      # every chunk's lock-step draws, in chunk order (patch.py:206-231)
        col = o.empty(Bh * Hh * Ww, 128)
        L.tcl_im2col3x3_small_f16(x_in, col, Bh, Hh, Ww, w["conv_in"][2], 128, stream())
        h = o.gemm(col, w["conv_in"][0], w["conv_in"][1])
        del col
        self._fl(2.0 * Hh * Ww * 9 * w["conv_in"][2] * 320, B, Bh)
        sizes = [(Hh, Ww)]
        skips = [(torch.cat([h, h]) if half else h, 320)]
        hh, ww, c = Hh, Ww, 320
        for i, co in enumerate(sd15.BLOCK_OUT):
            for j in range(2):
                first = half and i == 0 and j == 0
                h = self._resblock(f"down_blocks.{i}.resnets.{j}.", h, Bh if first else B, hh, ww, tproj, sw, rep=2 if first else 1)
                c = co
                if i < 3:
                    h = self._transformer(f"down_blocks.{i}.attentions.{j}.", h, B, Fs, hh, ww, text, sw, pair_half=first, kvi=kvi, ip=ip)
                skips.append((h, c))
            if i < 3:
                h, hh2, ww2 = o.conv3x3(h, B, hh, ww, c, *w[f"down{i}"], stride=2, pad=1)
                self._fl(2.0 * B * hh2 * ww2 * 9 * c * c)
                hh, ww = hh2, ww2
                sizes.append((hh, ww))
                skips.append((h, c))
        h = self._resblock("mid_block.resnets.0.", h, B, hh, ww, tproj, sw)
        h = self._transformer("mid_block.attentions.0.", h, B, Fs, hh, ww, text, sw, kvi=kvi, ip=ip)
        h = self._resblock("mid_block.resnets.1.", h, B, hh, ww, tproj, sw)
        level = 3
        for i, co in enumerate(sd15.BLOCK_OUT[::-1]):
            for j in range(3):
                sk, cs = skips.pop()
                h = self._resblock(f"up_blocks.{i}.resnets.{j}.", h, B, hh, ww, tproj, sw, skip=sk, cskip=cs)
                del sk
                if i > 0:
                    h = self._transformer(f"up_blocks.{i}.attentions.{j}.", h, B, Fs, hh, ww, text, sw, kvi=kvi, ip=ip)
            if i < 3:
                level -= 1
                h, hh2, ww2 = o.conv3x3(h, B, hh, ww, co, *w[f"up{i}"], up=sizes[level])   # nearest upsample fused in the gather
                self._fl(2.0 * B * hh2 * ww2 * 9 * co * co)
                hh, ww = hh2, ww2
        hn = o.groupnorm(h, 320, *w["norm_out"], B, hh * ww, 1e-5, True)
        eps, _, _ = o.conv3x3(hn, B, hh, ww, 320, *w["conv_out"])
        self._fl(2.0 * B * hh * ww * 9 * 320 * 4)
        return eps

    def forward_nhwc(self, x_in, F, Hh, Ww, t, text, ip=None):
        """One chunk: x_in [2F, Hh, Ww, 8] f16 -> eps [2F, Hh, Ww, 4] f16."""
        return self.forward_many(x_in, [F], Hh, Ww, t, text, ip=ip)
