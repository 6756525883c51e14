"""A synthetic CLIP vocabulary and a tiny text tower, shared by tests/test_text_host_cpu.py and tests/test_gpu_text.py: the two tokenizer files and
a `text_encoder/` directory written from the formats (independently of tc_light_amd's readers), the `transformers.CLIPTextModel` the engine is
compared with, and LoRA factors on that tower's modules.

The vocabulary: the 256 byte symbols of GPT-2's table (ids 0-255), the same with `</w>` (256-511), then one id per merge and the two special tokens
last.  The merges are seeded and in creation order (both halves of a merge exist before it, as in a trained BPE): the left half is a symbol without
`</w>`, the right half any symbol, both over lower-case letters, digits and punctuation; early merges are letter pairs, later ones build on them.
"""
import json
import os

import numpy as np
import torch

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
N_MERGES = 300
VOCAB_SIZE = 512 + N_MERGES + 2
# the tiny tower of the end-to-end tests; its token table has one row per id of the synthetic vocabulary
TINY = dict(width=128, layers=2, context_length=77, vocab_size=VOCAB_SIZE, heads=2, act="quick_gelu", eps=1e-5)


def byte_table():
    """byte -> printable stand-in character (GPT-2's bytes_to_unicode, restated): '!'-'~', U+00A1-U+00AC and U+00AE-U+00FF are themselves, the
    other bytes are U+0100, U+0101, ... in byte order."""
    own = [b for b in range(256) if 0x21 <= b <= 0x7E or 0xA1 <= b <= 0xAC or 0xAE <= b <= 0xFF]
    rest = [b for b in range(256) if b not in own]
    return {**{b: chr(b) for b in own}, **{b: chr(256 + i) for i, b in enumerate(rest)}}


def vocabulary(seed=3, n_merges=N_MERGES):
    """-> (token -> id, [(left, right)] in rank order)."""
    table = byte_table()
    vocab = {table[b]: b for b in range(256)}
    vocab.update({table[b] + "</w>": 256 + b for b in range(256)})
    g = np.random.default_rng(seed)
    letters = [c for i, c in enumerate("etaoinshrdlcumwfgypbvkjxqz") for _ in range(12 - i // 2 if i < 20 else 1)]     # common letters more often
    others = list("0123456789.,!?'-:;")
    lefts = letters + others
    rights = lefts + [c + "</w>" for c in lefts]
    merges = []
    while len(merges) < n_merges:
        a, b = lefts[g.integers(len(lefts))], rights[g.integers(len(rights))]
        if a + b in vocab:
            continue
        vocab[a + b] = len(vocab)
        merges.append((a, b))
        rights.append(a + b)                                             # a merged symbol can be merged again:
        if not (a + b).endswith("</w>"):                                 # one that ends a word only as a right half
            lefts.append(a + b)
    vocab[BOS], vocab[EOS] = len(vocab), len(vocab) + 1
    return vocab, merges


def write_tokenizer(d, config=False):
    """vocab.json + merges.txt (with the `#version` header line) in directory d; config: a tokenizer_config.json with model_max_length 77."""
    os.makedirs(d, exist_ok=True)
    vocab, merges = vocabulary()
    with open(os.path.join(d, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(os.path.join(d, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges))
    if config:
        with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
            json.dump({"model_max_length": 77}, f)
    return vocab, merges


def hf_config(arch):
    """The config.json of a transformers.CLIPTextModel of this architecture, written from transformers' field names."""
    w = arch["width"]
    return dict(hidden_size=w, intermediate_size=4 * w, num_hidden_layers=arch["layers"], num_attention_heads=arch["heads"],
                max_position_embeddings=arch["context_length"], vocab_size=arch["vocab_size"], hidden_act=arch["act"], layer_norm_eps=arch["eps"],
                projection_dim=w, bos_token_id=arch["vocab_size"] - 2, eos_token_id=arch["vocab_size"] - 1)


def hf_keys(sd, prefix="text_model."):
    """A state dict in OpenAI's names -> transformers.CLIPTextModel's, under `prefix` (restated here; tc_light_amd.clip.to_hf_text_state is tested
    against it)."""
    out = {prefix + "embeddings.token_embedding.weight": sd["token_embedding.weight"],
           prefix + "embeddings.position_embedding.weight": sd["positional_embedding"],
           prefix + "final_layer_norm.weight": sd["ln_final.weight"], prefix + "final_layer_norm.bias": sd["ln_final.bias"]}
    names = {"ln_1": "layer_norm1", "ln_2": "layer_norm2", "attn.out_proj": "self_attn.out_proj", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2"}
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))
    for i in range(layers):
        a, h = f"transformer.resblocks.{i}.", f"{prefix}encoder.layers.{i}."
        for kind in ("weight", "bias"):
            W = sd[a + "attn.in_proj_" + kind]
            n = W.shape[0] // 3
            for j, p in enumerate("qkv"):
                out[f"{h}self_attn.{p}_proj.{kind}"] = W[j * n:(j + 1) * n].clone()
            for x, y in names.items():
                out[f"{h}{y}.{kind}"] = sd[f"{a}{x}.{kind}"]
    return out


def hf_model(arch, hf_sd):
    """transformers.CLIPTextModel of the architecture in f32 on the CPU, loaded strictly from a `text_model.`-prefixed state dict (the prefix is
    dropped when the installed transformers' CLIPTextModel has no such level)."""
    from transformers import CLIPTextConfig, CLIPTextModel
    model = CLIPTextModel(CLIPTextConfig(**hf_config(arch))).eval()
    if not any(k.startswith("text_model.") for k in model.state_dict()):
        hf_sd = {k[len("text_model."):]: v for k, v in hf_sd.items()}
    model.load_state_dict({k: v.float() for k, v in hf_sd.items()}, strict=True)
    return model


def hidden(model, ids):
    with torch.no_grad():
        return model(input_ids=ids).last_hidden_state


def write_encoder(d, hf_sd, arch, name="model.safetensors", config=None):
    """A text_encoder/ directory: config.json (`config` overrides fields) and the weights as safetensors or, for pytorch_model.bin, torch.save."""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(hf_config(arch), **(config or {})), f)
    sd = {k: v.contiguous() for k, v in hf_sd.items()}
    if name.endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file(sd, os.path.join(d, name))
    else:
        torch.save(sd, os.path.join(d, name))


L0, L1 = "text_model.encoder.layers.0.", "text_model.encoder.layers.1."


def te_factors(arch, seed=11, gain=1.0):
    """[(module path, down, up, alpha)] on q_proj / v_proj / out_proj / fc1 of layer 0 and k_proj / fc2 of layer 1 (ranks 4 and 8, one alpha != r, one
    absent); up @ down has entries ~ gain / sqrt(fan_in), the size of the seeded weights themselves at gain 1 (tests/lora_sets.py's scaling)."""
    w = arch["width"]
    targets = [(L0 + "self_attn.q_proj", 4, w, w, 4.0), (L0 + "self_attn.v_proj", 4, w, w, 2.0), (L0 + "self_attn.out_proj", 8, w, w, None),
               (L0 + "mlp.fc1", 4, w, 4 * w, 4.0), (L1 + "self_attn.k_proj", 8, w, w, 8.0), (L1 + "mlp.fc2", 4, 4 * w, w, None)]
    g = np.random.default_rng(seed)
    out = []
    for path, r, fin, fout, alpha in targets:
        down = g.standard_normal((r, fin)) / np.sqrt(fin)
        up = g.standard_normal((fout, r)) * (gain / np.sqrt(r))
        out.append((path, torch.from_numpy(down.astype(np.float32)), torch.from_numpy(up.astype(np.float32)), alpha))
    return out


def merged_f32(hf_sd, fs, weight):
    """{key: W + weight * (alpha / r) * up @ down} in f32 over a copy of the prefixed state dict."""
    out = {k: v.clone() for k, v in hf_sd.items()}
    for path, down, up, alpha in fs:
        r = down.shape[0]
        out[path + ".weight"] = out[path + ".weight"].float() + weight * ((r if alpha is None else alpha) / r) * (up.float() @ down.float())
    return out
