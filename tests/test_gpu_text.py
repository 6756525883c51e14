"""GPU: prompt embeddings on the native CLIP engine (tc_light_amd/clip.py CLIPTextEngine, tc_light_amd/bpe.py, tc_light_amd/text.py): last_hidden_state
at the size of SD-1.5's text encoder against tests/golden/text.npz (transformers.CLIPTextModel in f32 on the CPU with the same seeded weights),
causality and batch independence bit for bit, and a tiny tower (tests/text_sets.py) through the whole public path -- directory, tokenizer, LoRA --
against transformers.CLIPTextModel run in the test."""
import os

import pytest
import torch

import lora_sets as S
import text_sets as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def G(golden):
    return golden("text")


@pytest.fixture(scope="module")
def engine(dev, G):
    from tc_light_amd.clip import SD15_TEXT, CLIPTextEngine, seeded_text_state_dict
    A = SD15_TEXT
    return CLIPTextEngine(seeded_text_state_dict(int(G["seed"]), **A), dev, heads=A["heads"], act=A["act"], eps=A["eps"])


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


# ---------------------------------------------------------------------------------------------------------------- the SD-1.5 size
def test_hidden_states_vs_golden(dev, engine, G):
    """last_hidden_state of three id rows in encode_prompt_inner's layout against transformers.CLIPTextModel in f32.  Bound: twice the f16 floor
    recorded with the golden (the same model with .half() on the CPU against its f32 self) -- one floor for the f16 weights, one for the f16
    activations, the margin of a whole tower in test_gpu_clip.py -- over all rows together and for every row on its own."""
    ids = torch.from_numpy(G["ids"])
    want = torch.from_numpy(G["last_hidden_state"])
    got = engine.hidden_states(ids)
    assert got.shape == (3, 77, 768) and got.dtype == torch.float16 and got.device.type == "cuda"
    got = got.float().cpu()
    assert torch.isfinite(got).all()
    floor = float(G["f16_floor"])
    rel = _rel(got, want)
    rows = (got - want).norm(dim=-1) / want.norm(dim=-1)
    print(f"last_hidden_state rel-L2 {rel:.3e}, worst row {float(rows.max()):.3e} at {divmod(int(rows.argmax()), 77)}, median row "
          f"{float(rows.median()):.3e} (floor {floor:.3e}, bound {2 * floor:.3e})")
    assert rel <= 2 * floor
    assert float(rows.max()) <= 2 * floor


def test_row_depends_on_earlier_ids_only(dev, engine, G):
    """The causal mask: other ids at positions >= 40 leave rows < 40 bit-identical and change every later row."""
    ids = torch.from_numpy(G["ids"])[:2].clone()
    other = ids.clone()
    other[:, 40:] = torch.randint(1000, 40000, (2, 37), generator=torch.Generator().manual_seed(9))
    assert not (other[:, 40:] == ids[:, 40:]).any()
    a, b = engine.hidden_states(ids).cpu(), engine.hidden_states(other).cpu()
    assert torch.equal(a[:, :40], b[:, :40])
    assert bool((a[:, 40:] != b[:, 40:]).any(-1).all())


def test_rows_do_not_depend_on_the_batch(dev, engine, G):
    """A chunk encoded alone and among three gives the same bits, and the same ids give the same bits twice."""
    ids = torch.from_numpy(G["ids"])
    all3 = engine.hidden_states(ids).cpu()
    for r in range(3):
        assert torch.equal(engine.hidden_states(ids[r:r + 1]).cpu()[0], all3[r]), r
    assert torch.equal(engine.hidden_states(ids).cpu(), all3)


def test_refusals(dev, engine, tmp_path, monkeypatch):
    """Ids outside the vocabulary, T = 0 and T = 78 are ValueErrors; a config.json the kernels do not cover is refused by field name before an engine
    is built or device memory allocated."""
    from tc_light_amd import clip, text
    ok = torch.full((1, 77), 5, dtype=torch.int64)
    for bad in (torch.full((1, 77), 49408), torch.full((1, 77), -1), torch.zeros(1, 0, dtype=torch.int64), torch.zeros(1, 78, dtype=torch.int64),
                torch.zeros(77, dtype=torch.int64)):
        with pytest.raises(ValueError):
            engine.hidden_states(bad)
    assert engine.hidden_states(ok[:, :1]).shape == (1, 1, 768)
    sd = clip.seeded_text_state_dict(5, **T.TINY)
    with pytest.raises(ValueError, match="5 heads"):
        clip.CLIPTextEngine(sd, dev, heads=5)
    with pytest.raises(ValueError, match="act"):
        clip.CLIPTextEngine(sd, dev, act="relu")

    def no_engine(*a, **k):
        raise AssertionError("an engine was built for a refused config")
    monkeypatch.setattr(clip.CLIPTextEngine, "__init__", no_engine)
    monkeypatch.setattr(text, "_ENC", {})
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for field, value in (("hidden_act", "relu"), ("num_attention_heads", 5)):
        d = str(tmp_path / field)
        T.write_encoder(d, clip.to_hf_text_state(sd), T.TINY, config={field: value})
        T.write_tokenizer(d)
        with pytest.raises(ValueError, match=field):
            text.encode_prompt_pair("soft light", "dark", dev, d)
    assert torch.cuda.memory_allocated() == before


# ---------------------------------------------------------------------------------------------------------------- a tiny tower, end to end
@pytest.fixture(scope="module")
def prompts():
    import yaml
    with open(os.path.join(ROOT, "configs", "tclight_default.yaml")) as f:
        g = yaml.safe_load(f)["generation"]
    return g["negative_prompt"], g["negative_prompt_t"]                  # four chunks with a ragged last one under the synthetic vocabulary, and one


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """The tiny tower in an SD snapshot's layout (text_encoder/ with prefixed keys as safetensors + config.json, tokenizer/ beside it) and its state
    dict in transformers' names."""
    from tc_light_amd.clip import seeded_text_state_dict
    root = tmp_path_factory.mktemp("snapshot")
    hf_sd = T.hf_keys(seeded_text_state_dict(5, **T.TINY))
    T.write_encoder(str(root / "text_encoder"), hf_sd, T.TINY)
    T.write_tokenizer(str(root / "tokenizer"), config=True)
    return str(root / "text_encoder"), hf_sd


def _reference(hf_sd, prompts, half=False):
    """encode_prompt_pair's chunking and tiling around transformers.CLIPTextModel on the CPU: f32, or .half() for the f16 floor."""
    from tc_light_amd.text import encode_prompt_inner, tile_and_concat
    model = T.hf_model(T.TINY, hf_sd)
    model = model.half() if half else model
    tok = _tok()
    c, uc = (encode_prompt_inner(p, tok, model, "cpu") for p in prompts)
    c, uc = tile_and_concat(c, uc)
    return torch.cat([uc, c]).float()


_TOK = {}


def _tok():
    import tempfile
    from tc_light_amd.bpe import CLIPBPE
    if "tok" not in _TOK:
        with tempfile.TemporaryDirectory() as d:
            T.write_tokenizer(d)
            _TOK["tok"] = CLIPBPE.from_dir(d)
    return _TOK["tok"]


@pytest.fixture()
def no_transformers_loaders(monkeypatch):
    import transformers

    def refuse(*a, **k):
        raise AssertionError("transformers' from_pretrained was called")
    monkeypatch.setattr(transformers.CLIPTextModel, "from_pretrained", classmethod(refuse))
    monkeypatch.setattr(transformers.CLIPTokenizer, "from_pretrained", classmethod(refuse))


def test_prompt_pair_through_the_public_path(dev, tiny, prompts, no_transformers_loaders, monkeypatch):
    """encode_prompt_pair(pos, neg, dev, enc_dir) on the tiny tower's directory: [2, 77 k, 128] f16 with k from the longer prompt, equal to
    transformers.CLIPTextModel in f32 on the same ids, tiled the same way, within twice that tower's own .half() floor; transformers' loaders
    are not called."""
    from tc_light_amd import text
    monkeypatch.setattr(text, "_ENC", {})
    enc_dir, hf_sd = tiny
    ref = _reference(hf_sd, prompts)
    floor = _rel(_reference(hf_sd, prompts, half=True), ref)
    k = -(-len(_tok()(prompts[0])["input_ids"]) // 75)
    assert k >= 3 and len(_tok()(prompts[0])["input_ids"]) % 75 and len(_tok()(prompts[1])["input_ids"]) <= 75
    out = text.encode_prompt_pair(prompts[0], prompts[1], dev, enc_dir)
    assert out.shape == (2, 77 * k, 128) and out.dtype == torch.float16 and out.device.type == "cuda" and out.is_contiguous()
    rel = _rel(out.cpu(), ref)
    print(f"tiny tower, {k} chunks: rel-L2 {rel:.3e} (its f16 floor {floor:.3e}, bound {2 * floor:.3e})")
    assert rel <= 2 * floor
    tok, enc = text.load_text_encoder(enc_dir, dev)
    assert type(tok).__name__ == "CLIPBPE" and tok.model_max_length == 77 and type(enc.engine).__name__ == "CLIPTextEngine"
    assert text.load_text_encoder(enc_dir, dev)[1] is enc                # cached
    assert torch.equal(text.encode_prompt_pair(prompts[0], prompts[1], dev, enc_dir), out)


@pytest.mark.parametrize("layout", ["kohya", "peft"])
def test_prompt_pair_with_a_text_encoder_lora(dev, tiny, prompts, layout, no_transformers_loaders, monkeypatch):
    """The same with a LoRA on the text encoder, named lora_te_... (kohya) or text_encoder.... (diffusers / PEFT): equal, within the same bound, to
    the f32 CPU model whose weights had weight * (alpha / r) * up @ down added in f32, and at least ten bounds away from the output without it.
    The LoRA weight 0.5 with factors of the weights' own size moves the CPU reference by far more than that, which is asserted first."""
    from tc_light_amd import lora as L, text
    monkeypatch.setattr(text, "_ENC", {})
    enc_dir, hf_sd = tiny
    fs, weight = T.te_factors(T.TINY), 0.5
    lora = L.LoRASet(L.load_lora(S.kohya((), fs) if layout == "kohya" else S.peft((), fs)), weight)
    assert L.has_part(lora.entries, "te") and not L.has_part(lora.entries, "unet") and len(lora.entries) == len(fs)
    merged = T.merged_f32(hf_sd, fs, weight)
    ref, ref0 = _reference(merged, prompts), _reference(hf_sd, prompts)
    floor = _rel(_reference(merged, prompts, half=True), ref)
    bound = 2 * floor
    moved = _rel(ref0, ref)
    assert moved >= 20 * bound, (moved, bound)                           # the CPU reference alone: the LoRA is far above what the test resolves
    out = text.encode_prompt_pair(prompts[0], prompts[1], dev, enc_dir, lora=lora).cpu()
    plain = text.encode_prompt_pair(prompts[0], prompts[1], dev, enc_dir).cpu()
    rel, away = _rel(out, ref), _rel(plain, out)
    print(f"{layout}: rel-L2 {rel:.3e} (floor {floor:.3e}, bound {bound:.3e}); without the LoRA {away:.3e} away (the references: {moved:.3e})")
    assert rel <= bound
    assert away >= 10 * bound
    # another LoRASet on the same directory reloads instead of serving the cached merge
    other = L.LoRASet(lora.entries, 0.25)
    assert not torch.equal(text.encode_prompt_pair(prompts[0], prompts[1], dev, enc_dir, lora=other).cpu(), out)
