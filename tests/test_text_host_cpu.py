"""CPU: the host side of the native prompt-embedding path: the key mapping of a text tower to and from transformers.CLIPTextModel, bpe.CLIPBPE against
transformers.CLIPTokenizer on a synthetic vocabulary (tests/text_sets.py), model_utils.load_text_state, and the absence of transformers from the
engine's sources."""
import glob
import json
import os
import re

import pytest
import torch
import yaml

import text_sets as T
from tc_light_amd import clip as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(width=64, layers=2, context_length=77, vocab_size=96, heads=1, act="quick_gelu", eps=1e-5)


# ---------------------------------------------------------------------------------------------------------------- key mapping
def test_text_state_round_trip_and_strict_load():
    """from_hf_text_state(to_hf_text_state(sd)) is sd bit for bit; both prefix layouts are read; position_ids is ignored; the mapping is the one
    written out in text_sets.hf_keys and loads into transformers.CLIPTextModel with strict=True."""
    sd = C.seeded_text_state_dict(4, **SMALL)
    assert set(sd) == set(C.text_param_shapes(**{k: SMALL[k] for k in ("width", "layers", "context_length", "vocab_size")}))
    assert "text_projection" not in sd and not any(k.startswith("visual.") for k in sd)
    hf = C.to_hf_text_state(sd)
    want = T.hf_keys(sd)
    assert set(hf) == set(want) and all(torch.equal(hf[k], want[k]) for k in hf)
    assert all(k.startswith("text_model.") for k in hf)
    bare = C.to_hf_text_state(sd, prefix="")
    assert set(bare) == {k[len("text_model."):] for k in hf}
    for layout in (hf, bare):
        for extra in ({}, {("text_model." if layout is hf else "") + "embeddings.position_ids": torch.arange(77)[None]}):
            back = C.from_hf_text_state({**layout, **extra})
            assert set(back) == set(sd)
            assert all(torch.equal(back[k], sd[k]) and back[k].dtype == sd[k].dtype for k in sd)
    assert set(C.with_text_prefix(bare)) == set(hf)
    with pytest.raises(KeyError, match="final_layer_norm"):
        C.from_hf_text_state({k: v for k, v in hf.items() if "final_layer_norm" not in k})
    model = T.hf_model(SMALL, hf)                                       # strict=True inside
    ids = torch.tensor([[94, 3, 17, 95, 95]])
    assert T.hidden(model, ids).shape == (1, 5, 64)
    # the seeded recipe of the full CLIP is unchanged by sharing it: same generator, same order
    assert C.SD15_TEXT == dict(width=768, layers=12, context_length=77, vocab_size=49408, heads=12, act="quick_gelu", eps=1e-5)
    assert C.to_hf_text_config(C.SD15_TEXT)["num_attention_heads"] == 12 and C.to_hf_text_config(C.SD15_TEXT)["intermediate_size"] == 3072


# ---------------------------------------------------------------------------------------------------------------- BPE
def _config_prompts():
    """Every prompt and negative prompt under configs/ (a prompt block is a string or a name -> string dictionary)."""
    out = []
    for p in sorted(glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True)):
        with open(p) as f:
            cfg = yaml.safe_load(f)
        for block in (cfg.get("generation") or {}, cfg.get("inversion") or {}):
            for k in ("prompt", "negative_prompt", "prompt_t", "negative_prompt_t"):
                v = block.get(k)
                out += [s for s in (v.values() if isinstance(v, dict) else [v]) if isinstance(s, str)]
    return out


CASES = ["a  b   c", "tab\tand\nnewline \r\n  runs\t\t", "   leading and trailing   ", "UPPER Case MiXed", "the cat's toy, she'll go, don't stop, I'm, we've, they're, he'd",
         "'s 'll don't DON'T", "route 66 in 2024, 3.14 and 1000000", "a1b22c", "wow!!! ... --- ?!?! (ok) [x] {y} #tag @me $5 50% a&b *c* ;:", "...,,,",
         "café naïve über straße", "光 明るい光 soft 光", "добрый СВЕТ", "cafe\u0301 and n\u0303 decomposed", "ÉCOLE İstanbul",
         "", "   ", "soft light <|endoftext|> warm light", "<|startoftext|>a photo<|endoftext|>", "<|endoftext|>", "emoji \U0001f600 and ² ½"]


def test_bpe_matches_transformers(tmp_path):
    """CLIPBPE and transformers.CLIPTokenizer, both from the same synthetic vocab.json / merges.txt, give the same ids on every prompt of configs/ and
    on CASES: whitespace runs, upper case, contractions, digits (each its own token), punctuation runs, accented / Cyrillic / CJK / emoji text
    (the byte path), decomposed accents (NFC), the empty string and literal special tokens.  No class of input is left out."""
    from transformers import CLIPTokenizer
    from tc_light_amd.bpe import CLIPBPE
    from tc_light_amd.text import encode_prompt_inner
    vocab, merges = T.write_tokenizer(str(tmp_path))
    assert len(vocab) == T.VOCAB_SIZE and len(merges) == T.N_MERGES
    hf = CLIPTokenizer.from_pretrained(str(tmp_path), model_max_length=77)
    mine = CLIPBPE.from_dir(str(tmp_path))
    assert (mine.bos_token_id, mine.eos_token_id, mine.model_max_length) == (hf.bos_token_id, hf.eos_token_id, 77) == (T.VOCAB_SIZE - 2, T.VOCAB_SIZE - 1, 77)
    prompts = _config_prompts()
    assert len(prompts) >= 8 and any(len(p) > 300 for p in prompts)
    # words spelled from the merged symbols themselves, alone and glued in pairs: these reach the merges of merges, where the rank order decides
    deep = [t.replace("</w>", "") for t, i in vocab.items() if 512 <= i < T.VOCAB_SIZE - 2 and len(t.replace("</w>", "")) >= 3]
    assert len(deep) >= 50
    spelled = [" ".join(deep), " ".join(a + b for a, b in zip(deep, deep[7:] + deep[:7])), "".join(deep[:40])]
    seen = set()
    for txt in prompts + CASES + spelled:
        want = hf(txt, truncation=False, add_special_tokens=False)["input_ids"]
        got = mine(txt, truncation=False, add_special_tokens=False)["input_ids"]
        assert got == want, repr(txt)
        seen.update(got)
    inv = {i: t for t, i in vocab.items()}
    merged = [inv[i] for i in seen if 512 <= i < T.VOCAB_SIZE - 2]
    assert len(merged) >= 30 and any(len(t.replace("</w>", "")) >= 3 for t in merged)          # merges fire, and merges of merges
    # each digit is its own token; NFC: the decomposed accent gives the ids of the composed one; a literal special is its id
    assert len(mine("2024")["input_ids"]) == 4
    assert mine("caf\u00e9")["input_ids"] == mine("cafe\u0301")["input_ids"] != mine("cafe")["input_ids"]
    assert mine("a <|endoftext|>")["input_ids"][-1] == mine.eos_token_id and mine("<|startoftext|>")["input_ids"] == [mine.bos_token_id]
    assert mine("") ["input_ids"] == [] and mine(" \n ")["input_ids"] == []
    with pytest.raises(ValueError, match="empty prompt"):
        encode_prompt_inner("", mine, None, "cpu")
    with pytest.raises(ValueError):
        mine("x", truncation=True)
    # clip.tokenize / tokenize_truncated take it as they take transformers' tokenizer
    long_ = " ".join(["light"] * 120)
    assert C.tokenize("soft light", mine, 77)[0].tolist() == C.tokenize("soft light", hf, 77)[0].tolist()
    assert C.tokenize_truncated(long_, mine)[0].tolist() == C.tokenize_truncated(long_, hf)[0].tolist()


def test_bpe_from_dir_and_load_tokenizer(tmp_path):
    """from_dir looks in d and d/tokenizer and needs both files; model_max_length comes from tokenizer_config.json when there is one; the text
    encoder's tokenizer is also found in the sibling ../tokenizer of an SD snapshot; clip.load_tokenizer keeps returning None for nothing."""
    from tc_light_amd.bpe import CLIPBPE
    from tc_light_amd import text
    assert CLIPBPE.from_dir(str(tmp_path)) is None and C.load_tokenizer(str(tmp_path)) is None and C.load_tokenizer("") is None
    T.write_tokenizer(str(tmp_path / "snap" / "tokenizer"), config=True)
    cfg = tmp_path / "snap" / "tokenizer" / "tokenizer_config.json"
    cfg.write_text(json.dumps({"model_max_length": 64}))
    for d in (tmp_path / "snap", tmp_path / "snap" / "tokenizer"):
        tok = C.load_tokenizer(str(d))
        assert isinstance(tok, CLIPBPE) and tok.model_max_length == 64
    os.makedirs(tmp_path / "snap" / "text_encoder")
    assert text.load_tokenizer(str(tmp_path / "snap" / "text_encoder")).model_max_length == 64
    os.remove(tmp_path / "snap" / "tokenizer" / "merges.txt")
    assert CLIPBPE.from_dir(str(tmp_path / "snap")) is None
    with pytest.raises(FileNotFoundError, match="tokenizer"):
        text.load_tokenizer(str(tmp_path / "snap" / "text_encoder"))


# ---------------------------------------------------------------------------------------------------------------- loading
def test_load_text_state(tmp_path):
    """model.safetensors before model.fp16.safetensors before pytorch_model.bin, each readable; both key layouts; FileNotFoundError naming the
    directory when there are no weights; config.json refusals name the field and come before the weights are looked for."""
    from tc_light_amd import model_utils as MU
    sd = C.seeded_text_state_dict(4, **SMALL)
    hf = C.to_hf_text_state(sd)
    other = {k: v + 1 for k, v in hf.items()}
    d = str(tmp_path / "enc")
    T.write_encoder(d, {**{k[len("text_model."):]: v for k, v in other.items()}, "embeddings.position_ids": torch.arange(77)[None]}, SMALL,
                    "pytorch_model.bin")
    got, opt = MU.load_text_state(d)                                    # the .bin alone, unprefixed keys, a position_ids buffer
    assert opt == dict(heads=1, act="quick_gelu", eps=1e-5)
    assert set(got) == set(hf) and all(torch.equal(got[k], other[k]) for k in hf)
    T.write_encoder(d, {k: v.half() for k, v in other.items()}, SMALL, "model.fp16.safetensors")
    got, _ = MU.load_text_state(d)                                      # fp16 safetensors before the .bin; returned as f32
    assert all(got[k].dtype == torch.float32 and torch.equal(got[k], other[k].half().float()) for k in hf)
    T.write_encoder(d, hf, SMALL, "model.safetensors")
    got, _ = MU.load_text_state(d)                                      # model.safetensors first
    assert all(torch.equal(got[k], hf[k]) for k in hf)
    back = C.from_hf_text_state(got)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    empty = tmp_path / "empty"
    os.makedirs(empty)
    (empty / "config.json").write_text(json.dumps(T.hf_config(SMALL)))
    with pytest.raises(FileNotFoundError, match=re.escape(str(empty))):
        MU.load_text_state(str(empty))
    for field, value in (("hidden_act", "relu"), ("num_attention_heads", 5), ("num_attention_heads", 8), ("layer_norm_eps", 1e-6),
                         ("intermediate_size", 128)):
        (empty / "config.json").write_text(json.dumps(dict(T.hf_config(SMALL), **{field: value})))
        with pytest.raises(ValueError, match=field):                    # before the missing weights are noticed
            MU.load_text_state(str(empty))
    T.write_encoder(d, hf, SMALL, "model.safetensors", config={"num_hidden_layers": 3})
    with pytest.raises(ValueError, match="num_hidden_layers"):
        MU.load_text_state(d)
    # absent fields are transformers' defaults (512 wide, 8 heads, a 2048-wide MLP): this 64-wide tower is then refused by hidden_size
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({}, f)
    with pytest.raises(ValueError, match="hidden_size"):
        MU.load_text_state(d)
    assert C.text_options(None)[0] == dict(heads=8, act="quick_gelu", eps=1e-5)
    assert C.text_options(C.to_hf_text_config(C.SD15_TEXT)) == (dict(heads=12, act="quick_gelu", eps=1e-5), dict(width=768, layers=12, context_length=77))


def test_missing_encoder_directory_still_means_stand_ins(tmp_path):
    from tc_light_amd.text import encode_prompt_pair
    with pytest.raises(FileNotFoundError):
        encode_prompt_pair("a", "b", "cpu", enc_dir=str(tmp_path / "no_clip"))
    with pytest.warns(UserWarning, match="stand-in"):
        out = encode_prompt_pair("a", "b", "cpu", enc_dir=str(tmp_path / "no_clip"), allow_random=True)
    assert out.shape == (2, 77, 768) and out.dtype == torch.float16


# ---------------------------------------------------------------------------------------------------------------- sources
def test_engine_sources_do_not_import_transformers():
    files = sorted(glob.glob(os.path.join(ROOT, "tc_light_amd", "*.py"))) + [os.path.join(ROOT, n) for n in ("run.py", "invert.py", "evaluate.py")]
    assert len(files) > 20
    pat = re.compile(r"import\s+transformers|from\s+transformers\b")    # anywhere: a lazy import inside a function counts
    bad = [os.path.relpath(p, ROOT) for p in files if pat.search(open(p, encoding="utf-8").read())]
    assert not bad, bad
