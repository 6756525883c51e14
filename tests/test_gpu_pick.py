"""GPU: pick-score (csrc/clip.hip's tcl_clip_preprocess_ld_u8 / tcl_pick_scores, tc_light_amd/clip.py's PickScore options, evaluate.py --pick): the
preprocess in the transformers processor's convention against PIL bit for bit, the padded patch rows, the scores kernel against numpy, one vision and
one text block with erf GELU and 16 heads against torch, the features and scores of the full ViT-H/14 architecture against tests/golden/pick.npz
(transformers.CLIPModel in f32 on the CPU with the same seeded weights), determinism, and the command line.  Needs the golden and PIL only."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16 = 2.0 ** -11            # half an ulp of f16, relative: the rounding error of one f16 store
MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def G(golden):
    return golden("pick")


@pytest.fixture(scope="module")
def engine(dev, G):
    """The full architecture (986 M seeded parameters), generated once for the module."""
    from tc_light_amd.clip import PICKSCORE_V1, arch_shapes, pick_engine, seeded_state_dict
    return pick_engine(seeded_state_dict(int(G["seed"]), **arch_shapes(PICKSCORE_V1)), dev)


@pytest.fixture(scope="module")
def one_layer(dev):
    """PickScore's widths and heads with one layer per tower: the blocks under test, and their f16 weights."""
    from tc_light_amd.clip import PICKSCORE_V1, arch_shapes, pick_engine, seeded_state_dict
    sd = seeded_state_dict(3, **dict(arch_shapes(PICKSCORE_V1), vision_layers=1, transformer_layers=1))
    return pick_engine(sd, dev)


class StoredIds:
    """The tokenizer interface tokenize_truncated reads, answering with the golden's id list."""
    def __init__(self, ids):
        from tc_light_amd.clip import EOT, SOT
        self.ids, self.bos_token_id, self.eos_token_id = [int(i) for i in ids], SOT, EOT

    def __call__(self, text, **kw):
        return {"input_ids": list(self.ids)}


def _rows(G):
    from tc_light_amd.clip import tokenize_truncated
    return [tokenize_truncated("", StoredIds(G[k])) for k in ("raw_ids_0", "raw_ids_1")]


def _L():
    from tc_light_amd.lib import lib, stream
    return lib(), stream()


def _rel(a, b):
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------------------------------- preprocess
def _frames(H, W, seed):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    smooth = np.asarray(Image.fromarray(small).resize((W, H), Image.BILINEAR))
    return np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), smooth])


def _pil_crop_floor(frame, side=224):
    """transformers' CLIP image processor up to the uint8 image: resize (short side `side`, long side int(side * long / short), PIL bicubic), then
    center_crop from (size - side) // 2 -- written out here, not taken from the code under test."""
    H, W = frame.shape[:2]
    short, long_ = min(H, W), max(H, W)
    nl = int(side * long_ / short)
    oh, ow = (nl, side) if W <= H else (side, nl)
    top, left = (oh - side) // 2, (ow - side) // 2
    return np.asarray(Image.fromarray(frame).resize((ow, oh), Image.BICUBIC))[top:top + side, left:left + side]


@pytest.mark.parametrize("H,W", [(720, 1280), (1280, 720), (227, 224), (224, 227), (448, 454), (333, 517)])
def test_preprocess_floor_matches_pil(dev, H, W):
    """Rule 1 at patch 14, ldp 640: the uint8 crop is PIL's resize(BICUBIC) + the (size - 224) // 2 crop bit for bit; columns 0..587 of the patch rows
    are (crop / 255 - mean) / std rounded to f16 in conv1.weight's column order and columns 588..639 are zero."""
    L, st = _L()
    fr = _frames(H, W, H + W)
    x = torch.from_numpy(fr).to(dev)
    N = len(fr)
    crop = torch.zeros(N, 224, 224, 3, dtype=torch.uint8, device=dev)
    patches = torch.full((N, 256, 640), float("nan"), dtype=torch.float16, device=dev)
    L.tcl_clip_preprocess_ld_u8(x, crop, patches, N, H, W, 224, 14, 640, 1, st)
    want = np.stack([_pil_crop_floor(f) for f in fr])
    got = crop.cpu().numpy()
    bad = int((got != want).sum())
    print(f"{H}x{W}: {bad} of {want.size} crop bytes differ from PIL; max |diff| {int(np.abs(got.astype(int) - want.astype(int)).max())}")
    assert bad == 0
    t = (torch.from_numpy(want).permute(0, 3, 1, 2).float().div(255) - MEAN) / STD
    rows = t.view(N, 3, 16, 14, 16, 14).permute(0, 2, 4, 1, 3, 5).reshape(N, 256, 588).half()
    p = patches.cpu()
    assert torch.equal(p[..., :588], rows)
    assert torch.equal(p[..., 588:], torch.zeros(N, 256, 52, dtype=torch.float16))
    # the patch rows alone give the same bytes
    patches2 = torch.full_like(patches, float("nan"))
    L.tcl_clip_preprocess_ld_u8(x, 0, patches2, N, H, W, 224, 14, 640, 1, st)
    assert torch.equal(patches2.cpu(), p)


@pytest.mark.parametrize("H,W", [(720, 1280), (227, 224), (333, 517)])
def test_preprocess_ld_rule0_is_the_old_entry(dev, H, W):
    """With rule 0 and ldp = 3 * patch^2 the new entry reproduces tcl_clip_preprocess_u8 byte for byte."""
    L, st = _L()
    fr = _frames(H, W, H * W)
    x = torch.from_numpy(fr).to(dev)
    N = len(fr)
    out = []
    for new in (False, True):
        crop = torch.zeros(N, 224, 224, 3, dtype=torch.uint8, device=dev)
        patches = torch.zeros(N, 49, 3072, dtype=torch.float16, device=dev)
        if new:
            L.tcl_clip_preprocess_ld_u8(x, crop, patches, N, H, W, 224, 32, 3072, 0, st)
        else:
            L.tcl_clip_preprocess_u8(x, crop, patches, N, H, W, 224, 32, st)
        out.append((crop.cpu(), patches.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_geometry_rule_c_side_agrees(dev):
    from tc_light_amd.clip import resize_geometry_rule
    L, _ = _L()
    g = (ctypes.c_int * 4)()
    for H, W in [(720, 1280), (1280, 720), (227, 224), (224, 227), (448, 454), (480, 853), (301, 224), (100, 60), (333, 517)]:
        for rule, name in ((0, "round"), (1, "floor")):
            L.tcl_clip_resize_geometry_rule(H, W, 224, rule, g)
            assert tuple(g) == resize_geometry_rule(H, W, 224, name), (H, W, name)
    with pytest.raises(RuntimeError):
        L.tcl_clip_resize_geometry_rule(227, 224, 224, 2, g)


def test_preprocess_ld_refuses_bad_arguments(dev):
    L, st = _L()
    x = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=dev)
    out = torch.zeros(1, 256, 640, dtype=torch.float16, device=dev)
    for ldp, rule in ((600, 1), (576, 1), (512, 1), (640, 2), (640, -1)):          # not a multiple of 64, below 3 * 14 * 14, unknown rule
        with pytest.raises(RuntimeError):
            L.tcl_clip_preprocess_ld_u8(x, 0, out, 1, 64, 64, 224, 14, ldp, rule, st)


# ---------------------------------------------------------------------------------------------------------------- scores
def test_pick_scores_kernel_vs_numpy(dev):
    """exp(logit_scale) cos(text, feat_i) and their mean against numpy in f64; a second call gives the same bits."""
    from tc_light_amd.clip import pick_scores
    rng = np.random.default_rng(4)
    f = rng.standard_normal((37, 1024)).astype(np.float32); t = rng.standard_normal(1024).astype(np.float32)
    ls = np.float32(math.log(100.0))
    f64, t64 = f.astype(np.float64), t.astype(np.float64)
    want = math.exp(float(ls)) * (f64 @ t64) / (np.linalg.norm(f64, axis=1) * np.linalg.norm(t64))
    fd, td = torch.from_numpy(f).to(dev), torch.from_numpy(t).to(dev)
    mean, per = pick_scores(fd, td, float(ls))
    print(f"max |per-image - numpy| {np.abs(per - want).max():.3e}, |mean - numpy| {abs(mean - want.mean()):.3e}")
    assert per.dtype == np.float64 and per.shape == (37,)
    assert np.abs(per - want).max() < 1e-11 and abs(mean - want.mean()) < 1e-11        # f64 sums of 1024 products in another order, values up to 100
    mean2, per2 = pick_scores(fd, td, float(ls))
    assert mean2 == mean and np.array_equal(per2, per)
    one = pick_scores(fd[:1], td, float(ls))
    assert one[0] == one[1][0] == per[0]
    with pytest.raises(ValueError):
        pick_scores(fd, td[:512], float(ls))


# ---------------------------------------------------------------------------------------------------------------- blocks
def _block_ref(x, p, B, T, heads, causal, act):
    """ResidualAttentionBlock / CLIPEncoderLayer in f32 on the device from the engine's f16 weights and the same f16 input."""
    F = torch.nn.functional
    W = x.shape[1]
    w = {k: v.float() for k, v in p.items()}
    x = x.float()
    h = F.layer_norm(x, (W,), w["ln_1.weight"], w["ln_1.bias"], 1e-5)
    q, k, v = F.linear(h, w["attn.in_proj_weight"], w["attn.in_proj_bias"]).view(B, T, 3, heads, W // heads).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(W // heads)
    if causal:
        s = s + torch.full((T, T), float("-inf"), device=x.device).triu(1)
    a = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * T, W)
    x = x + F.linear(a, w["attn.out_proj.weight"], w["attn.out_proj.bias"])
    u = F.linear(F.layer_norm(x, (W,), w["ln_2.weight"], w["ln_2.bias"], 1e-5), w["mlp.c_fc.weight"], w["mlp.c_fc.bias"])
    u = F.gelu(u) if act == "gelu" else u * torch.sigmoid(1.702 * u)
    return x + F.linear(u, w["mlp.c_proj.weight"], w["mlp.c_proj.bias"])


@pytest.mark.parametrize("tower", ["vision", "text"])
def test_block_vs_torch(dev, one_layer, tower):
    """One block with erf GELU and 16 heads (vision: width 1280, d = 80, T = 257; text: width 1024, d = 64, T = 20, causal) against torch in f32 from
    the same f16 input and weights.  The engine stores eight f16 tensors on the way (ln_1, qkv, the probabilities, the attention output, the first
    residual sum, ln_2, gelu(c_fc), the result), each a relative error of at most 2^-11 of a tensor the result depends on with a gain of about one:
    the bound on the relative L2 error is their sum, 8 x 2^-11 = 3.9e-3.  The same reference with QuickGELU, or with width // 64 heads, is farther
    from it than that (asserted: the test can see either mistake)."""
    e = one_layer
    tw, B, T, causal = (e.visual, 2, 257, False) if tower == "vision" else (e.text, 3, 20, True)
    assert tw.heads == 16 and e.act == "gelu"
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B * T, tw.width, generator=g).half().to(dev)
    got = e._blocks(x, tw, B, T, causal).float()
    ref = _block_ref(x, tw.layers[0], B, T, 16, causal, "gelu")
    rel = _rel(got, ref)
    wrong_act = _rel(_block_ref(x, tw.layers[0], B, T, 16, causal, "quick_gelu"), ref)
    wrong_heads = _rel(_block_ref(x, tw.layers[0], B, T, 20 if tower == "vision" else 8, causal, "gelu"), ref)
    print(f"{tower} block: rel-L2 {rel:.3e} (bound {8 * U16:.3e}); the reference with QuickGELU is {wrong_act:.3e} away, with the other head count "
          f"{wrong_heads:.3e}")
    assert torch.isfinite(got).all()
    assert wrong_act > 8 * U16 and wrong_heads > 8 * U16
    assert rel <= 8 * U16


def test_encode_text_short_row_is_the_padded_rows_eot(dev, engine, G):
    """encode_text on the unpadded [1, T] row (T < 77) against the same ids zero-padded to 77: the tower is causal, so the EOT row does not see the
    padding and the two are the same number computed twice.  Only the tiling of the kernels differs with the row count, so they agree far inside the
    f16 floor of the text feature; a tower that was not causal, or positional rows that were not the first T, would differ in the first digit."""
    row = _rows(G)[0]
    T = row.shape[1]
    assert T < 77
    padded = torch.zeros(1, 77, dtype=torch.int64)
    padded[0, :T] = row[0]
    a, b = engine.encode_text(row).cpu(), engine.encode_text(padded).cpu()
    rel = _rel(a, b)
    print(f"T = {T}: rel-L2 between the unpadded and the padded call {rel:.3e} (text floor {float(G['f16_floor_text']):.3e})")
    assert rel <= float(G["f16_floor_text"])
    with pytest.raises(ValueError):
        engine.encode_text(torch.zeros(1, 78, dtype=torch.int64))
    with pytest.raises(ValueError):
        engine.encode_text(torch.zeros(1, 0, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------- features and scores
def _features(engine, G):
    v = torch.cat([engine.encode_image(torch.from_numpy(G[k])) for k in ("frames_a", "frames_b")])
    t = torch.cat([engine.encode_text(r) for r in _rows(G)])
    return v, t


def test_features_vs_golden(dev, engine, G):
    """encode_image / encode_text at the full architecture against transformers.CLIPModel in f32.  Bound: twice the f16 floor recorded with the
    golden (the same model with .half() on the CPU against its f32 self), as for ViT-B/32: the engine rounds at more points than torch's half path.
    Floors: image 1.43e-3, text 1.83e-3.  No measured value is recorded here yet: this test has not been run on an MI355X."""
    v, t = _features(engine, G)
    v, t = v.cpu(), t.cpu()
    fi, ft = float(G["f16_floor_image"]), float(G["f16_floor_text"])
    ri, rt = _rel(v, torch.from_numpy(G["image_features"])), _rel(t, torch.from_numpy(G["text_features"]))
    print(f"image features rel-L2 {ri:.3e} (floor {fi:.3e}, bound {2 * fi:.3e}); text features rel-L2 {rt:.3e} (floor {ft:.3e}, bound {2 * ft:.3e})")
    assert v.shape == (len(G["frames_a"]) + len(G["frames_b"]), 1024) and t.shape == (2, 1024)
    assert _rows(G)[1].shape == (1, 77) and len(G["raw_ids_1"]) > 75                   # the long prompt went in truncated
    assert ri <= 2 * fi
    assert rt <= 2 * ft


def test_scores_vs_golden(dev, engine, G):
    """pick-score of both golden clips under both prompts, per image and averaged.  A cosine of unit vectors moves by at most the sum of their
    relative errors, so |delta| <= exp(logit_scale) (b_img + b_txt) with b the feature bounds above (twice the golden's floors): 0.093, where the two
    clips are 12.7 apart."""
    from tc_light_amd.clip import pick_scores
    from tc_light_amd.evaluate import pick_score
    assert abs(engine.logit_scale - float(G["logit_scale"])) < 1e-6
    tol = math.exp(float(G["logit_scale"])) * (2 * float(G["f16_floor_image"]) + 2 * float(G["f16_floor_text"]))
    na = len(G["frames_a"])
    v, t = _features(engine, G)
    for p in range(2):
        for c, sl in enumerate((slice(0, na), slice(na, None))):
            mean, per = pick_scores(v[sl], t[p], engine.logit_scale)
            d = np.abs(per - G["scores"][p, sl]).max()
            print(f"prompt {p} clip {c}: pick-score {mean:.5f} (golden {G['pick_score'][p, c]:.5f}), max per-image |diff| {d:.3e}, tolerance {tol:.3e}")
            assert abs(mean - float(G["pick_score"][p, c])) <= tol
            assert d <= tol
    # the public function: the same number from frames and a prompt
    for c, key in enumerate(("frames_a", "frames_b")):
        s = pick_score(torch.from_numpy(G[key]), "", engine, StoredIds(G["raw_ids_0"]))
        assert abs(s - float(G["pick_score"][0, c])) <= tol
    assert abs(float(G["pick_score"][0, 0]) - float(G["pick_score"][0, 1])) >= 10 * tol


def test_pick_score_is_deterministic(dev, engine, G):
    """Two runs of the whole figure (preprocess, both towers, the scores kernel) give identical bits."""
    from tc_light_amd.evaluate import pick_score
    frames = torch.from_numpy(G["frames_b"])
    with pytest.warns(UserWarning):
        a = pick_score(frames, "soft warm light from the left", engine, None, allow_random=True)
        b = pick_score(frames, "soft warm light from the left", engine, None, allow_random=True)
    assert a == b and math.isfinite(a)
    assert torch.equal(engine.encode_image(frames), engine.encode_image(frames))
    feats = engine.encode_image(frames)
    with pytest.warns(UserWarning):
        assert pick_score(frames, "soft warm light from the left", engine, None, allow_random=True, features=feats) == a


# ---------------------------------------------------------------------------------------------------------------- the command line
def _run_dir(tmp_path):
    import yaml
    from tc_light_amd.dataparser import write_mjpeg_avi
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (1, 150, 220, 3), dtype=np.uint8)
    src = np.stack([np.roll(base[0], (k, 2 * k), (0, 1)) for k in range(4)])
    edit = np.clip(src[:, 5:135, 7:205].astype(np.int32) + 20, 0, 255).astype(np.uint8)
    write_mjpeg_avi(str(tmp_path / "output.avi"), edit)
    write_mjpeg_avi(str(tmp_path / "output_gt.avi"), src)
    cfg = {"generation": {"prompt": {"a": "soft light", "b": "warm light from the left window"}}, "models": {"raft": str(tmp_path / "absent.pth")}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))


def _evaluate(tmp_path, *args):
    env = dict(os.environ, TCL_ALLOW_RANDOM_WEIGHTS="1")
    r = subprocess.run(["timeout", "-k", "10", "140", sys.executable, os.path.join(ROOT, "evaluate.py"), "--output_dir", str(tmp_path), *args],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    blocks = r.stdout.split("unknown_video - ")[1:]
    assert len(blocks) == 2
    vals = [dict(ln.split(": ") for ln in b.splitlines()[1:] if ": " in ln) for b in blocks]
    lines = (tmp_path / "result.txt").read_text().splitlines()
    assert lines[0] == "unknown_video - warm light from the left window"
    return [ln for ln in r.stdout.splitlines() if "not computed here" in ln], [ln.split(": ")[0] for ln in lines[1:]], vals


def test_evaluate_cli_with_pick(dev, tmp_path):
    """evaluate.py --pick <absent path> with random weights allowed: result.txt carries pick-score and warp-error-ssim, the note names clip-frame and
    clip-text only, and the two prompts' blocks differ in pick-score."""
    _run_dir(tmp_path)
    note, keys, vals = _evaluate(tmp_path, "--pick", str(tmp_path / "absent_pick"))
    assert len(note) == 1 and "clip-frame, clip-text" in note[0] and "pick-score" not in note[0]
    assert keys == ["pick-score", "warp-error-ssim"]
    assert vals[0]["warp-error-ssim"] == vals[1]["warp-error-ssim"] and vals[0]["pick-score"] != vals[1]["pick-score"]
    assert all(len(v["pick-score"].split(".")[1]) == 4 and abs(float(v["pick-score"])) <= math.exp(math.log(1 / 0.07)) + 1e-3 for v in vals)


def test_evaluate_cli_with_clip_and_pick(dev, tmp_path):
    """With --clip too: the reference's four figures between them, in its order, and no "not computed" line."""
    _run_dir(tmp_path)
    note, keys, vals = _evaluate(tmp_path, "--pick", str(tmp_path / "absent_pick"), "--clip", str(tmp_path / "absent_clip.pt"))
    assert note == []
    assert keys == ["clip-frame", "clip-text", "pick-score", "warp-error-ssim"]
    assert vals[0]["clip-frame"] == vals[1]["clip-frame"] and vals[0]["clip-text"] != vals[1]["clip-text"]
    assert vals[0]["pick-score"] != vals[1]["pick-score"]
