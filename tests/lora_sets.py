"""One seeded set of LoRA factors on SD-1.5 UNet modules, shared by tests/test_lora_host_cpu.py and tests/test_gpu_lora.py: the factors, the two
file layouts users have (written here from the formats, independently of tc_light_amd/lora.py's reader) and the merge W + weight*(alpha/r)*up@down
in float64.

Targets: to_q / to_k / to_v / to_out.0 of an attn1 (rank 4) and of an attn2 (rank 16, to_k / to_v read the 768-wide text), a GEGLU ff.net.0.proj
(rank 4, alpha 2: alpha != r), a proj_in as a 1x1 convolution pair and a proj_out as a linear pair (rank 16), a ResBlock conv1 as LoCon
(down [r, in, 3, 3], up [out, r, 1, 1]) and conv_in with 4 input channels (no alpha, like attn2.to_v).
"""
import numpy as np
import torch

A1 = "down_blocks.0.attentions.0.transformer_blocks.0.attn1."
A2 = "mid_block.attentions.0.transformer_blocks.0.attn2."
# (module path in the UNet's key names, down shape, up shape, alpha or None)
TARGETS = ([(A1 + n, (4, 320), (320, 4), 4.0) for n in ("to_q", "to_k", "to_v", "to_out.0")]
           + [(A2 + "to_q", (16, 1280), (1280, 16), 16.0), (A2 + "to_k", (16, 768), (1280, 16), 16.0), (A2 + "to_v", (16, 768), (1280, 16), None),
              (A2 + "to_out.0", (16, 1280), (1280, 16), 16.0),
              ("down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj", (4, 640), (5120, 4), 2.0),
              ("up_blocks.1.attentions.0.proj_in", (16, 1280, 1, 1), (1280, 16, 1, 1), 16.0),
              ("up_blocks.3.attentions.2.proj_out", (16, 320), (320, 16), 8.0),
              ("down_blocks.0.resnets.0.conv1", (4, 320, 3, 3), (320, 4, 1, 1), 4.0),
              ("conv_in", (4, 4, 3, 3), (320, 4, 1, 1), None)])


def factors(seed=2024, gain=1.0):
    """[(path, down, up, alpha)] f32; up @ down has entries ~ gain / sqrt(fan_in): the size of the seeded weights themselves at gain 1."""
    g = np.random.default_rng(seed)
    out = []
    for path, ds, us, alpha in TARGETS:
        fan_in = int(np.prod(ds[1:]))
        down = g.standard_normal(ds) / np.sqrt(fan_in)
        up = g.standard_normal(us) * (gain / np.sqrt(ds[0]))
        out.append((path, torch.from_numpy(down.astype(np.float32)), torch.from_numpy(up.astype(np.float32)), alpha))
    return out


def kohya(fs, te=()):
    """lora_unet_<path with _>.lora_down.weight / .lora_up.weight / .alpha (a 0-dim tensor); `te`: the same for lora_te_."""
    d = {}
    for prefix, part in (("lora_unet_", fs), ("lora_te_", te)):
        for path, down, up, alpha in part:
            m = prefix + path.replace(".", "_")
            d[m + ".lora_down.weight"], d[m + ".lora_up.weight"] = down, up
            if alpha is not None:
                d[m + ".alpha"] = torch.tensor(float(alpha))
    return d


def peft(fs, te=(), old_attn=False):
    """unet.<path>.lora_A.weight / .lora_B.weight / .alpha; `old_attn`: the attention projections in the older
    `<attn>.processor.to_q_lora.down.weight` spelling (to_out.0 -> to_out_lora)."""
    d = {}
    for root, part in (("unet.", fs), ("text_encoder.", te)):
        for path, down, up, alpha in part:
            head, _, leaf = path.rpartition(".")
            if leaf == "0" and head.endswith("to_out"):
                head, leaf = head[:-len(".to_out")], "to_out.0"
            if old_attn and root == "unet." and leaf in ("to_q", "to_k", "to_v", "to_out.0"):
                m = f"{root}{head}.processor.{leaf.split('.')[0]}_lora"
                d[m + ".down.weight"], d[m + ".up.weight"] = down, up
            else:
                m = root + path
                d[m + ".lora_A.weight"], d[m + ".lora_B.weight"] = down, up
            if alpha is not None:
                d[m + ".alpha"] = torch.tensor(float(alpha))
    return d


def product64(down, up):
    """up @ down contracted over the rank in float64, and |up| @ |down| (what bounds the f32 rounding of that product), shaped [out, in, kh, kw]
    for a convolution pair and [out, in] for a linear one."""
    d, u = down.double(), up.double().flatten(1)
    shape = (u.shape[0],) + tuple(d.shape[1:])
    return (u @ d.flatten(1)).reshape(shape), (u.abs() @ d.abs().flatten(1)).reshape(shape)


def merged64(sd, fs, weight=1.0):
    """{key: W + weight*(alpha/r)*up@down in float64} for the keys the set touches (conv_in: its first 4 input channels)."""
    out = {}
    for path, down, up, alpha in fs:
        k = path + ".weight"
        r = down.shape[0]
        p, _ = product64(down, up)
        W = out.get(k, sd[k].double()).clone()
        s = weight * ((r if alpha is None else alpha) / r)
        if k == "conv_in.weight":
            W[:, :4] += s * p
        else:
            W += s * p.reshape(W.shape)
        out[k] = W
    return out
