"""CPU: `generation.use_lora` / `generation.lora` on the host -- tc_light_amd/lora.py (the two file layouts, the f32 merge), its place in
`model_utils.load_unet_state` (base -> 8-channel conv_in -> IC-Light offsets -> LoRA) and the refusals of `run.main`.

The merge is checked against W + weight*(alpha/r)*up@down computed independently in float64 (tests/lora_sets.py).  Bound, per element, from the
f32 operations the merge is specified to do (u = 2^-24, gamma_n = n*u / (1 - n*u), P = |up| @ |down|, s = weight*alpha/r):
    fl(up @ down)        errs by at most gamma_r * P                       (r products and r-1 additions per element, any summation order)
    s -> f32, s * (...)  two more roundings of that product                -> |s| * gamma_(r+2) * P, taken as gamma_(r+3) to cover second order
    W + (...)            the stored f32 result carries one rounding of its own: u * |W'|, which no f32 merge can avoid
so |got - exact| <= |s| * gamma_(r+3) * P + u * |exact|.  Every tensor is seeded.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import lora_sets as S
from tc_light_amd import lora as L
from tc_light_amd import model_utils, sd15

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def touched_keys(fs):
    return [p + ".weight" for p, *_ in fs]


@pytest.fixture(scope="module")
def fs():
    return S.factors()


@pytest.fixture(scope="module")
def unet_sd(fs):
    """Every key of the engine's UNet layout (so that kohya's underscore names are resolved against the real key list); seeded values for the
    tensors the set touches, empty placeholders for the other 680-odd (the merge must not look at them)."""
    shapes = sd15.unet_param_shapes()
    want = set(touched_keys(fs))
    assert want <= set(shapes)
    real = sd15.random_state_dict({k: shapes[k] for k in sorted(want)}, seed=1)
    return {k: real[k] if k in want else torch.empty(0) for k in shapes}


def same_entries(a, b):
    assert [e[0] for e in a] == [e[0] for e in b]
    for (_, da, ua, aa), (_, db, ub, ab) in zip(a, b):
        assert torch.equal(da, db) and torch.equal(ua, ub) and da.shape == db.shape and ua.shape == ub.shape and aa == ab


def test_layouts_parse_to_the_same_entries(fs, tmp_path):
    from safetensors.torch import save_file
    ref = L.load_lora(S.kohya(fs))
    assert len(ref) == len(S.TARGETS) and all(e[0].startswith("lora_unet_") for e in ref)
    by_name = {e[0]: e for e in ref}
    for path, down, up, alpha in fs:                                    # nothing lost or reordered on the way
        _, d, u, a = by_name["lora_unet_" + path.replace(".", "_")]
        assert torch.equal(d, down) and torch.equal(u, up) and a == alpha
    assert sum(e[3] is None for e in ref) == 2 and any(e[3] is not None and e[3] != e[1].shape[0] for e in ref)
    assert {e[1].shape[0] for e in ref} == {4, 16}
    same_entries(ref, L.load_lora(S.peft(fs)))
    same_entries(ref, L.load_lora(S.peft(fs, old_attn=True)))
    # the same through files: a .safetensors path, and a directory plus lora_weight_name
    for name, d in (("k.safetensors", S.kohya(fs)), ("p.safetensors", S.peft(fs))):
        save_file({k: v.contiguous() for k, v in d.items()}, str(tmp_path / name))
        same_entries(ref, L.load_lora(str(tmp_path / name)))
        same_entries(ref, L.load_lora(str(tmp_path), weight_name=name))
    with pytest.raises(FileNotFoundError):
        L.load_lora(str(tmp_path))                                      # a directory without a file name
    with pytest.raises(FileNotFoundError):
        L.load_lora(str(tmp_path / "absent.safetensors"))


@pytest.mark.parametrize("layout", ["kohya", "peft"])
@pytest.mark.parametrize("weight", [1.0, 0.75])
def test_merge_equals_float64_product_within_f32_rounding(fs, unet_sd, layout, weight):
    entries = L.load_lora(getattr(S, layout)(fs))
    sd = L.merge_into(dict(unet_sd), entries, weight)
    exact = S.merged64(unet_sd, fs, weight)
    assert set(exact) == set(touched_keys(fs))
    for path, down, up, alpha in fs:
        k = path + ".weight"
        r = down.shape[0]
        s = weight * ((r if alpha is None else alpha) / r)
        _, P = S.product64(down, up)
        bound = abs(s) * gamma(r + 3) * P
        if k == "conv_in.weight":
            bound = torch.cat([bound, torch.zeros_like(bound)], 1)      # channels 4-7 are not touched at all
        bound = bound.reshape(exact[k].shape) + U * exact[k].abs()
        err = (sd[k].double() - exact[k]).abs()
        assert sd[k].dtype == torch.float32 and sd[k].shape == unet_sd[k].shape
        assert bool((err <= bound).all()), (k, float((err / bound.clamp_min(1e-300)).max()))
        assert float((sd[k] - unet_sd[k]).abs().max()) > 0                # and it is not the unmerged weight
    untouched = [k for k in unet_sd if k not in exact]
    assert all(sd[k] is unet_sd[k] for k in untouched)
    assert torch.equal(sd["conv_in.weight"][:, 4:], unet_sd["conv_in.weight"][:, 4:])


# ------------------------------------------------------------------------------------------------ the loader: a small layout through the real code
def _mini_layout(fs):
    full = sd15.unet_param_shapes()
    keys = touched_keys(fs) + ["conv_in.bias", S.A1 + "to_out.0.bias", "down_blocks.0.resnets.0.conv2.weight", "conv_norm_out.weight"]
    return {k: full[k] for k in keys}


@pytest.fixture
def mini(fs, monkeypatch):
    shapes = _mini_layout(fs)
    monkeypatch.setattr(sd15, "unet_param_shapes", lambda in_channels=8: dict(shapes))
    return shapes


def _write_pair(tmp_path, shapes):
    from safetensors.torch import save_file
    base = sd15.random_state_dict({k: ((320, 4, 3, 3) if k == "conv_in.weight" else s) for k, s in shapes.items()}, seed=11)
    off = sd15.random_state_dict(shapes, seed=12, gain=0.01)
    pu, po = str(tmp_path / "unet.safetensors"), str(tmp_path / "iclight_sd15_fc.safetensors")
    save_file({k: v.half() for k, v in base.items()}, pu)
    save_file({k: v.half() for k, v in off.items()}, po)
    return pu, po, base, off


def test_no_lora_and_zero_weight_leave_the_loader_output_bit_identical(fs, mini, tmp_path):
    pu, po, _, _ = _write_pair(tmp_path, mini)
    zero = {"pretrained_model_name_or_path_or_dict": S.kohya(fs), "lora_weight": 0.0}
    for load in (lambda **kw: model_utils.load_unet_state(pu, po, **kw), lambda **kw: model_utils.load_unet_state(None, None, allow=True, **kw)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                              # the seeded stand-in path warns; not this test's subject
            parent, none, w0 = load(), load(lora=None), load(lora=zero)
        assert list(parent) == list(none) == list(w0)
        for k in parent:
            assert parent[k].dtype == none[k].dtype == w0[k].dtype
            assert torch.equal(parent[k], none[k]) and torch.equal(parent[k], w0[k]), k
            assert torch.equal(parent[k].view(torch.int32), w0[k].view(torch.int32)), k          # the bits, signed zeros included


def test_lora_is_merged_after_the_offsets_and_conv_in_keeps_channels_4_to_7(fs, mini, tmp_path):
    pu, po, base, off = _write_pair(tmp_path, mini)
    block = {"pretrained_model_name_or_path_or_dict": S.peft(fs), "lora_weight_name": None, "lora_adapter": "style", "lora_weight": 0.5}
    parent = model_utils.load_unet_state(pu, po)
    got = model_utils.load_unet_state(pu, po, lora=block)
    # the loader's own steps restated: widen, add the offsets in f32, then the LoRA on top of THAT (in float64 here)
    w8 = torch.zeros(320, 8, 3, 3)
    w8[:, :4] = base["conv_in.weight"]
    assert torch.equal(parent["conv_in.weight"], w8 + off["conv_in.weight"])
    exact = S.merged64(parent, fs, 0.5)
    for k in parent:
        if k in exact:
            assert float((got[k].double() - exact[k]).abs().max()) <= 1e-6 * float(exact[k].abs().max()), k      # coarse here; the tight bound is above
            assert not torch.equal(got[k], parent[k])
        else:
            assert torch.equal(got[k], parent[k]), k
    assert torch.equal(got["conv_in.weight"][:, 4:], off["conv_in.weight"][:, 4:])               # zero widening + offset, untouched by the 4-channel LoRA
    assert not torch.equal(got["conv_in.weight"][:, :4], parent["conv_in.weight"][:, :4])
    # the seeded stand-in path (no checkpoint, allow_random) takes the LoRA as well: that is what the GPU parity test loads
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r0 = model_utils.load_unet_state(None, None, allow=True)
        r1 = model_utils.load_unet_state(None, None, allow=True, lora=L.from_config(block))
    assert not torch.equal(r0[S.A2 + "to_v.weight"], r1[S.A2 + "to_v.weight"]) and torch.equal(r0["conv_in.bias"], r1["conv_in.bias"])


# ------------------------------------------------------------------------------------------------ refusals
def test_unknown_target_rank_and_shape_mismatch_are_refused(fs, unet_sd):
    good = S.kohya(fs)
    stray = dict(good)
    for n in ("lora_unet_down_blocks_9_attentions_0_proj_in", "lora_unet_mid_block_attentions_0_transformer_blocks_0_attn3_to_q",
              "lora_unet_time_embedding_linear_3", "lora_unet_up_blocks_0_attentions_0_proj_in"):      # up block 0 has no attention in SD-1.5
        stray[n + ".lora_down.weight"], stray[n + ".lora_up.weight"] = torch.zeros(4, 320), torch.zeros(320, 4)
    before = {k: v.clone() for k, v in unet_sd.items() if v.numel()}
    sd = dict(unet_sd)
    with pytest.raises(KeyError) as e:
        L.merge_into(sd, L.load_lora(stray))
    msg = str(e.value)
    assert msg.count("lora_unet_") == 3 and "lora_unet_down_blocks_9_attentions_0_proj_in" in msg and "+1 more" in msg
    assert all(sd[k] is unet_sd[k] for k in sd) and all(torch.equal(unet_sd[k], v) for k, v in before.items())     # nothing was written
    q = "lora_unet_" + (S.A1 + "to_q").replace(".", "_")
    for slot, t in ((".lora_up.weight", torch.zeros(320, 8)),                 # rank of up != rank of down
                    (".lora_down.weight", torch.zeros(4, 300)),               # in-features do not fit
                    (".lora_up.weight", torch.zeros(640, 4)),                 # out-features do not fit
                    (".lora_up.weight", torch.zeros(320, 4, 3, 3))):          # a convolution up on a linear down
        bad = dict(good)
        bad[q + slot] = t
        with pytest.raises(ValueError):
            L.merge_into(dict(unet_sd), L.load_lora(bad))
    bad = dict(good)
    bad["lora_unet_conv_in.lora_down.weight"] = torch.zeros(4, 5, 3, 3)        # neither 8 nor the 4 latent channels
    with pytest.raises(ValueError):
        L.merge_into(dict(unet_sd), L.load_lora(bad))
    with pytest.raises(KeyError, match="neither"):
        L.load_lora(dict(good, **{"some.other.tensor": torch.zeros(1)}))
    half = {k: v for k, v in good.items() if k != q + ".lora_up.weight"}
    with pytest.raises(ValueError, match="both"):
        L.load_lora(half)
    with pytest.raises(ValueError):
        L.from_config(None)
    with pytest.raises(ValueError):
        L.from_config({"lora_weight": 1.0})


@pytest.mark.parametrize("case,exc", [("no block", ValueError), ("missing file", FileNotFoundError), ("directory, missing file", FileNotFoundError)])
def test_run_use_lora_without_block_or_file_raises_before_models(tmp_path, monkeypatch, case, exc):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.lora was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    lora_yaml = {"no block": "",
                 "missing file": f", lora: {{pretrained_model_name_or_path_or_dict: {tmp_path / 'absent.safetensors'}, lora_weight_name: null, lora_weight: 1.0}}",
                 "directory, missing file": f", lora: {{pretrained_model_name_or_path_or_dict: {tmp_path}, lora_weight_name: absent.safetensors}}"}[case]
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{scene_type: video, height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}, use_lora: true{lora_yaml}}}
""")
    with pytest.raises(exc):
        run.main(["--config", str(cfg)])


# ------------------------------------------------------------------------------------------------ text encoder, at the state-dict level
TE = "text_model.encoder.layers.0."


def _te_factors():
    g = np.random.default_rng(5)
    t = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32) * 0.1)
    return [(TE + "self_attn.q_proj", t(4, 32), t(32, 4), 2.0), (TE + "self_attn.out_proj", t(4, 32), t(32, 4), None), (TE + "mlp.fc1", t(4, 32), t(128, 4), 4.0)]


class _TinyTE(torch.nn.Module):
    """The module names of an HF CLIP text model, one layer, width 32."""

    def __init__(self):
        super().__init__()
        lin = torch.nn.Linear
        layer = torch.nn.Module()
        layer.self_attn = torch.nn.Module()
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            setattr(layer.self_attn, n, lin(32, 32))
        layer.mlp = torch.nn.Module()
        layer.mlp.fc1, layer.mlp.fc2 = lin(32, 128), lin(128, 32)
        self.text_model = torch.nn.Module()
        self.text_model.encoder = torch.nn.Module()
        self.text_model.encoder.layers = torch.nn.ModuleList([layer])


def test_text_encoder_entries_merge_into_its_state_dict_only(fs, unet_sd, monkeypatch):
    from tc_light_amd import text
    te = _te_factors()
    a, b = L.load_lora(S.kohya(fs, te)), L.load_lora(S.peft(fs, te, old_attn=True))
    same_entries(a, b)
    assert L.has_part(a, "te") and L.has_part(a, "unet") and not L.has_part(L.load_lora(S.kohya(fs)), "te")
    assert sum(e[0].startswith("lora_te_text_model_encoder_layers_0_") for e in a) == 3
    # the older text-encoder spelling: to_q_lora -> q_proj, to_out_lora -> out_proj
    old = {f"text_encoder.{TE}self_attn.to_q_lora.down.weight": te[0][1], f"text_encoder.{TE}self_attn.to_q_lora.up.weight": te[0][2],
           f"text_encoder.{TE}self_attn.to_out_lora.down.weight": te[1][1], f"text_encoder.{TE}self_attn.to_out_lora.up.weight": te[1][2]}
    assert [e[0] for e in L.load_lora(old)] == ["lora_te_text_model_encoder_layers_0_self_attn_out_proj", "lora_te_text_model_encoder_layers_0_self_attn_q_proj"]
    torch.manual_seed(0)
    model = _TinyTE()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    text.merge_text_lora(model, L.LoRASet(a, 0.5))                       # the UNet entries of the same file are not this state dict's business
    after = model.state_dict()
    exact = S.merged64(before, te, 0.5)
    for k in before:
        if k in exact:
            _, down, up, alpha = [f for f in te if f[0] + ".weight" == k][0]
            s = 0.5 * ((4 if alpha is None else alpha) / 4)
            assert bool(((after[k].double() - exact[k]).abs() <= s * gamma(4 + 3) * S.product64(down, up)[1] + U * exact[k].abs()).all()), k
            assert not torch.equal(after[k], before[k])
        else:
            assert torch.equal(after[k], before[k]), k
    # ... and the UNet merge skips the lora_te_ entries instead of calling them unknown
    sd = L.merge_into(dict(unet_sd), a, 1.0)
    assert not torch.equal(sd[S.A1 + "to_q.weight"], unet_sd[S.A1 + "to_q.weight"])
    with pytest.raises(KeyError, match="lora_te_"):
        L.merge_into({"text_model.embeddings.token_embedding.weight": torch.zeros(4, 4)}, a, 1.0, part="te")
    # the deterministic stand-in embeddings have no encoder: said once, and the embeddings are the ones without a LoRA
    monkeypatch.setattr(text, "_WARNED_TE_LORA", False)
    with pytest.warns(UserWarning, match="text-encoder entries"):
        c1 = text.encode_prompt_pair("warm light", "dark", "cpu", None, allow_random=True, lora=L.LoRASet(a, 1.0))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        c2 = text.encode_prompt_pair("warm light", "dark", "cpu", None, allow_random=True, lora=L.LoRASet(a, 1.0))
        c3 = text.encode_prompt_pair("warm light", "dark", "cpu", None, allow_random=True)
    assert not any("text-encoder entries" in str(w.message) for w in rec)
    assert torch.equal(c1, c2) and torch.equal(c1, c3)
