"""Prompt embeddings (reference: generate.py:98-135 encode_prompt_inner / encode_prompt_pair).

Host plumbing, outside the two hot paths.  `encode_prompt_inner(txt, tokenizer, text_encoder, device)` is the reference's chunked
scheme on any tokenizer / encoder with the HF CLIP interface (`tokenizer(txt, truncation=False, add_special_tokens=False)["input_ids"]`,
`.model_max_length`, `.bos_token_id`, `.eos_token_id`; `text_encoder(ids).last_hidden_state`): untruncated tokens -> chunks of
model_max_length-2 wrapped in BOS/EOS, padded with EOS to model_max_length -> last_hidden_state per chunk.  `encode_prompt_pair` tiles the
shorter side, concatenates the chunks along the sequence and returns cat([uncond, cond]) (generate.py:553-555).
`load_text_encoder(dir)` loads SD-1.5's text encoder (the text tower of CLIP ViT-L/14) from a local directory into clip.CLIPTextEngine, the
HIP engine of the CLIP figures read at last_hidden_state, and its tokenizer into bpe.CLIPBPE; a missing directory raises unless random
stand-ins were explicitly allowed (model_utils.allow_random), in which case deterministic text-seeded embeddings of the right shape are used.
A LoRA's text-encoder entries (`lora_te_...` / `text_encoder....`, tc_light_amd/lora.py) are merged into the local checkpoint's state dict in
f32 before it is cast to f16; the stand-in embeddings have no weights to merge into, which is said once in a warning.
"""
import hashlib
import math
import os
import warnings
from types import SimpleNamespace

import numpy as np
import torch

_ENC = {}
_WARNED_TE_LORA = False


def encode_prompt_inner(txt, tokenizer, text_encoder, device):
    """A4 (generate.py:98-114): the untruncated token stream laid out as an id matrix [n_chunks, model_max_length] -- column 0 is BOS, the
    next model_max_length-2 columns carry the stream row after row, every other cell (the closing column and the ragged end of the
    last row) is EOS -- and encoded in one batch -> last_hidden_state [n_chunks, model_max_length, hidden]."""
    width = int(tokenizer.model_max_length)
    body = width - 2
    stream = torch.as_tensor(list(tokenizer(txt, truncation=False, add_special_tokens=False)["input_ids"]), dtype=torch.int64)
    rows = -(-int(stream.numel()) // body)
    if rows == 0:
        raise ValueError("empty prompt: the reference's chunking yields no chunk to encode (generate.py:108-112)")
    cells = torch.full((rows * body,), int(tokenizer.eos_token_id), dtype=torch.int64)
    cells[:stream.numel()] = stream
    ids = torch.full((rows, width), int(tokenizer.eos_token_id), dtype=torch.int64)
    ids[:, 0] = int(tokenizer.bos_token_id)
    ids[:, 1:1 + body] = cells.view(rows, body)
    with torch.no_grad():
        return text_encoder(ids.to(device)).last_hidden_state


def tile_and_concat(c, uc):
    """A4 (generate.py:116-135): both embeddings get the chunk count of the longer prompt -- the shorter one cycles through its chunks --
    and the chunks become one sequence.  c, uc: [n_chunks, L, D] -> ([1, k*L, D], [1, k*L, D])."""
    k = max(c.shape[0], uc.shape[0])

    def as_sequence(e):
        cycled = e.repeat(-(-k // e.shape[0]), 1, 1).narrow(0, 0, k)
        return cycled.reshape(1, k * e.shape[1], e.shape[2])

    return as_sequence(c), as_sequence(uc)


def merge_text_lora(text_encoder, lora):
    """The lora_te_ entries of `lora` (lora.LoRASet) merged into an HF-CLIP-shaped module's weights, f32 on the host."""
    from . import lora as L
    sd = {k: (v.detach().float().cpu() if v.is_floating_point() else v) for k, v in text_encoder.state_dict().items()}
    text_encoder.load_state_dict(L.merge_into(sd, lora.entries, lora.weight, part="te"))
    return text_encoder


class TextEncoder:
    """clip.CLIPTextEngine behind the call encode_prompt_inner makes: `encoder(ids).last_hidden_state` [B, T, width] f16 on the device."""

    def __init__(self, engine):
        self.engine = engine

    def __call__(self, ids):
        return SimpleNamespace(last_hidden_state=self.engine.hidden_states(ids))


def load_tokenizer(enc_dir):
    """bpe.CLIPBPE from `enc_dir`, its `tokenizer` sub-directory or, in the layout of an SD snapshot, the sibling `../tokenizer`."""
    from .bpe import CLIPBPE
    tried = (enc_dir, os.path.join(os.path.dirname(os.path.abspath(enc_dir)), "tokenizer"))
    for d in tried:
        tok = CLIPBPE.from_dir(d)
        if tok is not None:
            return tok
    raise FileNotFoundError(f"no CLIP tokenizer (vocab.json + merges.txt) in {tried[0]!r}, its `tokenizer` sub-directory or {tried[1]!r}")


def load_text_encoder(enc_dir, dev, lora=None):
    """-> (bpe.CLIPBPE, TextEncoder) for the `text_encoder/` directory of an SD-1.5 snapshot.  The LoRA's text-encoder entries are merged into the
    f32 state dict in transformers' key names (the names LoRA files spell) before it is renamed and packed: one f16 rounding, like the UNet's."""
    from . import clip, lora as L
    from .model_utils import load_text_state
    te_lora = lora if lora is not None and L.has_part(lora.entries, "te") else None
    key = (enc_dir, te_lora is not None)
    # the cache entry holds the LoRASet it was merged with (so the object stays alive and `is` cannot meet a recycled id); another set reloads
    if key not in _ENC or _ENC[key][2] is not te_lora:
        tok = load_tokenizer(enc_dir)
        sd, options = load_text_state(enc_dir)
        if te_lora is not None:
            sd = L.merge_into(sd, te_lora.entries, te_lora.weight, part="te")
        _ENC[key] = (tok, TextEncoder(clip.CLIPTextEngine(clip.from_hf_text_state(sd), dev, **options)), te_lora)
    return _ENC[key][:2]


def _n_chunks_proxy(txt):
    return max(1, math.ceil(len(txt.replace(",", " , ").replace(".", " . ").split()) * 1.3 / 75))


def _stand_in(txt, dev):
    n = _n_chunks_proxy(txt)
    seed = int.from_bytes(hashlib.sha256(txt.encode()).digest()[:4], "little")
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 77, 768)).astype(np.float32)).to(dev).half()


def _encode_chunks(texts, dev, enc_dir, allow_random, tokenizer, text_encoder, lora):
    """The chunked embedding [n_chunks, L, D] of every text, on the CLIP engine or -- no checkpoint and allow_random -- as stand-ins."""
    global _WARNED_TE_LORA
    if tokenizer is None and enc_dir and os.path.isdir(enc_dir):
        tokenizer, text_encoder = load_text_encoder(enc_dir, dev, lora)
    if tokenizer is not None:
        return [encode_prompt_inner(t, tokenizer, text_encoder, dev) for t in texts]
    else:
        if not allow_random:
            raise FileNotFoundError(f"CLIP text encoder directory {enc_dir!r} not found (models.text_encoder); set models.allow_random / "
                                    "TCL_ALLOW_RANDOM_WEIGHTS=1 for deterministic stand-in embeddings")
        warnings.warn("CLIP text encoder not found -> deterministic text-seeded stand-in embeddings (allow_random)")
        if lora is not None and not _WARNED_TE_LORA:
            from . import lora as L
            if L.has_part(lora.entries, "te"):
                _WARNED_TE_LORA = True
                warnings.warn("the LoRA carries text-encoder entries (lora_te_ / text_encoder.), but the stand-in embeddings have no text "
                              "encoder to merge them into: they are not applied")
        return [_stand_in(t, dev) for t in texts]


def encode_prompt_pair(positive, negative, dev, enc_dir=None, allow_random=False, tokenizer=None, text_encoder=None, lora=None):
    """-> [2, L*k, 768] f16 = cat([uncond, cond]) (generate.py:553-555).  `lora` (lora.LoRASet): its text-encoder entries are merged into
    the checkpoint under `enc_dir`; a tokenizer / text_encoder handed in is used as it is."""
    c, uc = _encode_chunks([positive, negative], dev, enc_dir, allow_random, tokenizer, text_encoder, lora)
    c, uc = tile_and_concat(c, uc)
    return torch.cat([uc, c]).to(torch.float16).contiguous()


def encode_prompt_set(positives, negative, dev, enc_dir=None, allow_random=False, tokenizer=None, text_encoder=None, lora=None):
    """generation.prompt_path: the keyframe prompts and the one negative, each encoded once exactly as encode_prompt_pair encodes its two, and all
    brought to the chunk count of the longest (tile_and_concat's cycling) so that they can be blended element by element.
    -> (uncond [L*k, 768], conds [P, L*k, 768]) f16; with one prompt they are the two halves of encode_prompt_pair, bit for bit."""
    embs = _encode_chunks(list(positives) + [negative], dev, enc_dir, allow_random, tokenizer, text_encoder, lora)
    longest = max(embs, key=lambda e: e.shape[0])
    seqs = [tile_and_concat(e, longest)[0] for e in embs]
    return seqs[-1][0].to(torch.float16).contiguous(), torch.cat(seqs[:-1]).to(torch.float16).contiguous()
