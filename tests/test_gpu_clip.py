"""GPU: the CLIP engine behind clip-frame / clip-text (csrc/clip.hip, tc_light_amd/clip.py, evaluate.py --clip): the preprocess kernel against PIL bit
for bit, the short-sequence attention kernel against torch, QuickGELU and the embedding rows, the features and the two figures against
tests/golden/clip.npz (transformers.CLIPModel in f32 on the CPU with the same seeded weights), determinism, and the command line."""
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


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def G(golden):
    return golden("clip")


@pytest.fixture(scope="module")
def engine(dev, G):
    from tc_light_amd.clip import CLIPEngine, seeded_state_dict
    return CLIPEngine(seeded_state_dict(int(G["seed"])), dev)


def _L():
    from tc_light_amd.lib import lib, stream
    return lib(), stream()


# ---------------------------------------------------------------------------------------------------------------- preprocess
def _frames(H, W, seed):
    """One random and one smooth uint8 frame (the smooth one has long runs where the bicubic taps overshoot little; the random one clips)."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    smooth = np.asarray(Image.fromarray(small).resize((W, H), Image.BILINEAR))
    return np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), smooth])


def _pil_crop(frame, side=224):
    from tc_light_amd.clip import resize_geometry
    oh, ow, top, left = resize_geometry(*frame.shape[:2], side)
    return np.asarray(Image.fromarray(frame).resize((ow, oh), Image.BICUBIC))[top:top + side, left:left + side]


@pytest.mark.parametrize("H,W", [(720, 1280), (1280, 720), (360, 640), (160, 200), (224, 224), (333, 517)])
def test_preprocess_matches_pil(dev, H, W):
    """The uint8 crop is PIL's resize(BICUBIC) + centre crop bit for bit; the f16 patch rows are (crop / 255 - mean) / std (f32, as ToTensor and
    Normalize compute it) rounded to f16, in conv1.weight's column order."""
    L, st = _L()
    fr = _frames(H, W, H + W)
    x = torch.from_numpy(fr).to(dev)
    N = len(fr)
    crop = torch.zeros(N, 224, 224, 3, dtype=torch.uint8, device=dev)
    patches = torch.zeros(N, 49, 3072, dtype=torch.float16, device=dev)
    L.tcl_clip_preprocess_u8(x, crop, patches, N, H, W, 224, 32, st)
    want = np.stack([_pil_crop(f) for f in fr])
    got = crop.cpu().numpy()
    bad = int((got != want).sum())
    print(f"{H}x{W}: {bad} of {want.size} crop bytes differ from PIL; max |diff| {int(np.abs(got.astype(int) - want.astype(int)).max())}")
    assert bad == 0
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)
    t = (torch.from_numpy(want).permute(0, 3, 1, 2).float().div(255) - mean) / std
    rows = t.view(N, 3, 7, 32, 7, 32).permute(0, 2, 4, 1, 3, 5).reshape(N, 49, 3072).half()
    assert torch.equal(patches.cpu(), rows)
    # either output alone gives the same bytes
    crop2 = torch.zeros_like(crop); patches2 = torch.zeros_like(patches)
    L.tcl_clip_preprocess_u8(x, crop2, 0, N, H, W, 224, 32, st)
    L.tcl_clip_preprocess_u8(x, 0, patches2, N, H, W, 224, 32, st)
    assert torch.equal(crop2, crop) and torch.equal(patches2, patches)


def test_resize_geometry_c_side_agrees(dev):
    import ctypes
    from tc_light_amd.clip import resize_geometry
    L, _ = _L()
    g = (ctypes.c_int * 4)()
    for H, W in [(720, 1280), (1280, 720), (224, 224), (333, 517), (160, 200), (300, 225), (1080, 1920), (225, 224), (481, 227)]:
        L.tcl_clip_resize_geometry(H, W, 224, g)
        assert tuple(g) == resize_geometry(H, W), (H, W)


def test_preprocess_refuses_bad_arguments(dev):
    L, st = _L()
    x = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=dev)
    out = torch.zeros(1, 49, 3072, dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError):
        L.tcl_clip_preprocess_u8(x, 0, 0, 1, 64, 64, 224, 32, st)                       # no output
    with pytest.raises(RuntimeError):
        L.tcl_clip_preprocess_u8(x, 0, out, 1, 64, 64, 224, 30, st)                      # 224 % 30


# ---------------------------------------------------------------------------------------------------------------- attention
def _attn_ref(qkv, B, T, H, d, causal):
    q, k, v = qkv.float().view(B, T, 3, H, d).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    if causal:
        s = s + torch.full((T, T), float("-inf")).triu(1)
    return (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * T, H * d)


@pytest.mark.parametrize("d,T,H,causal", [(64, 50, 12, False), (64, 50, 3, True), (64, 77, 8, True), (64, 77, 2, False), (80, 257, 2, False),
                                          (80, 257, 1, True), (64, 1, 2, False), (64, 288, 1, True)])
def test_attention_vs_torch(dev, d, T, H, causal):
    """softmax(q k^T / sqrt(d) (+ mask)) v against torch in f32 on the same f16-rounded inputs.  The kernel rounds the probabilities and the output
    to f16, each a relative error of at most 2^-11: the bound on the relative L2 error is their sum, 2^-10."""
    L, st = _L()
    B = 3
    g = torch.Generator().manual_seed(d * 1000 + T + int(causal))
    qkv = (torch.randn(B * T, 3 * H * d, generator=g) * 1.5).half()
    out = torch.full((B * T, H * d), float("nan"), dtype=torch.float16, device=dev)
    L.tcl_clip_attention_f16(qkv.to(dev), out, B, T, H, d, 1.0 / math.sqrt(d), int(causal), st)
    ref = _attn_ref(qkv, B, T, H, d, causal)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    rel = float((got - ref).norm() / ref.norm())
    print(f"d={d} T={T} H={H} causal={causal}: rel-L2 {rel:.3e} (bound {2 * U16:.3e}), max |diff| {float((got - ref).abs().max()):.3e}")
    assert rel <= 2 * U16


def test_attention_causal_ignores_later_keys(dev):
    """With the mask, keys and values after position i have no influence on row i: perturbing rows >= 40 of K and V leaves rows < 40 bit-identical
    (and changes later rows); without the mask every row changes."""
    L, st = _L()
    B, T, H, d = 2, 77, 8, 64
    W = H * d
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, T, 3 * W, generator=g).half()
    other = qkv.clone()
    other[:, 40:, W:] = torch.randn(B, T - 40, 2 * W, generator=g).half()
    outs = {}
    for causal in (1, 0):
        for name, x in (("a", qkv), ("b", other)):
            o = torch.empty(B * T, W, dtype=torch.float16, device=dev)
            L.tcl_clip_attention_f16(x.to(dev).view(B * T, 3 * W), o, B, T, H, d, 0.125, causal, st)
            outs[causal, name] = o.view(B, T, W).cpu()
    assert torch.equal(outs[1, "a"][:, :40], outs[1, "b"][:, :40])
    assert not torch.equal(outs[1, "a"][:, 40:], outs[1, "b"][:, 40:])
    assert not torch.equal(outs[0, "a"][:, :40], outs[0, "b"][:, :40])


def test_attention_refuses_unsupported_shapes(dev):
    L, st = _L()
    x = torch.zeros(400 * 3 * 128, dtype=torch.float16, device=dev)
    for T, d in ((289, 64), (77, 40), (77, 136), (0, 64)):
        with pytest.raises(RuntimeError):
            L.tcl_clip_attention_f16(x, x, 1, T, 1, d, 0.125, 0, st)


# ---------------------------------------------------------------------------------------------------------------- QuickGELU, embed
def test_quick_gelu_vs_torch(dev):
    """x * sigmoid(1.702 x) in f32, rounded once: within one f16 ulp of torch's f32 result rounded to f16 (the fast exponential differs in the last bits)."""
    L, st = _L()
    g = torch.Generator().manual_seed(2)
    x = torch.cat([torch.randn(4096, generator=g) * 3, torch.linspace(-12, 12, 4096)]).half()
    y = torch.empty_like(x, device=dev)
    L.tcl_clip_quick_gelu_f16(x.to(dev), y, x.numel(), st)
    ref = x.float() * torch.sigmoid(1.702 * x.float())
    err = (y.float().cpu() - ref).abs()
    assert bool((err <= 2 * U16 * ref.abs() + 2.0 ** -24).all()), float((err / (ref.abs() + 1e-6)).max())


def test_embed_vs_torch(dev):
    L, st = _L()
    g = torch.Generator().manual_seed(3)
    B, T, W, V = 3, 50, 768, 1000
    patch = torch.randn(B, T - 1, W, generator=g).half(); cls = torch.randn(W, generator=g).half(); pos = torch.randn(T, W, generator=g).half()
    gamma = (1 + 0.1 * torch.randn(W, generator=g)).half(); beta = (0.1 * torch.randn(W, generator=g)).half()
    out = torch.empty(B * T, W, dtype=torch.float16, device=dev)
    L.tcl_clip_embed_f16(patch.to(dev), cls.to(dev), 0, 0, pos.to(dev), gamma.to(dev), beta.to(dev), out, B, T, W, 0, 1e-5, st)
    x = torch.cat([cls.float().expand(B, 1, W), patch.float()], 1) + pos.float()
    ref = torch.nn.functional.layer_norm(x, (W,), gamma.float(), beta.float(), 1e-5).view(B * T, W)
    err = (out.float().cpu() - ref).abs()
    # one f16 rounding of an f32 LayerNorm whose statistics are summed in another order: an ulp of the result plus 1e-5 of the normalised value
    assert bool((err <= 2 * U16 * ref.abs() + 1e-4).all()), float(err.max())
    # the text rows: table[id] + pos, one rounding -- exact
    table = torch.randn(V, 512, generator=g).half(); tpos = torch.randn(77, 512, generator=g).half()
    ids = torch.randint(0, V, (B, 77), generator=g, dtype=torch.int32)
    tout = torch.empty(B * 77, 512, dtype=torch.float16, device=dev)
    L.tcl_clip_embed_f16(0, 0, ids.to(dev), table.to(dev), tpos.to(dev), 0, 0, tout, B, 77, 512, V, 1e-5, st)
    assert torch.equal(tout.cpu().view(B, 77, 512), (table[ids.long()].float() + tpos.float()).half())


# ---------------------------------------------------------------------------------------------------------------- features and figures
def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_features_vs_golden(dev, engine, G):
    """encode_image / encode_text against transformers.CLIPModel in f32.  Bound: twice the f16 floor recorded with the golden (the same model with
    .half() on the CPU against its f32 self): the engine rounds at more points than torch's half path (the patch rows, the probabilities)."""
    v = engine.encode_image(torch.from_numpy(G["frames"])).cpu()
    t = engine.encode_text(torch.from_numpy(G["ids"])).cpu()
    fi, ft = float(G["f16_floor_image"]), float(G["f16_floor_text"])
    ri, rt = _rel(v, torch.from_numpy(G["image_features"])), _rel(t, torch.from_numpy(G["text_features"]))
    print(f"image features rel-L2 {ri:.3e} (floor {fi:.3e}, bound {2 * fi:.3e}); text features rel-L2 {rt:.3e} (floor {ft:.3e}, bound {2 * ft:.3e})")
    assert v.shape == (len(G["frames"]), 512) and t.shape == (2, 512)
    assert ri <= 2 * fi
    assert rt <= 2 * ft
    # batching does not change a frame's feature by more than the GEMM tile choice can (same summation order per element: identical)
    v1 = engine.encode_image(torch.from_numpy(G["frames"]), batch=3).cpu()
    assert _rel(v1, v) <= 2 * fi


def test_scores_vs_golden(dev, engine, G):
    """clip-frame and clip-text of the two golden clips.  The cosine of two unit vectors with relative error e each is off by at most about 2 e, so
    the absolute tolerance is 4 x the f16 floor of the golden: floor = max(image, text) ~ 1.4e-3 -> 5.6e-3 (the two clips differ by > 100 x that)."""
    from tc_light_amd.evaluate import clip_frame
    from tc_light_amd.clip import scores
    tol = 4 * max(float(G["f16_floor_image"]), float(G["f16_floor_text"]))
    ns = int(G["n_static"])
    frames = torch.from_numpy(G["frames"])
    t = engine.encode_text(torch.from_numpy(G["ids"]))
    for c, clip_frames in enumerate((frames[:ns], frames[ns:])):
        feats = engine.encode_image(clip_frames)
        cf = clip_frame(clip_frames, engine)
        ct = scores(feats, t[0])[1]
        print(f"clip {c}: clip-frame {cf:.5f} (golden {G['clip_frame'][c]:.5f}), clip-text {ct:.5f} (golden {G['clip_text'][0, c]:.5f}), tolerance {tol:.2e}")
        assert abs(cf - float(G["clip_frame"][c])) <= tol
        assert abs(ct - float(G["clip_text"][0, c])) <= tol
        assert abs(scores(feats, t[1])[1] - float(G["clip_text"][1, c])) <= tol


def test_scores_kernel_vs_numpy(dev):
    from tc_light_amd.clip import scores
    rng = np.random.default_rng(4)
    f = rng.standard_normal((37, 512)).astype(np.float32); t = rng.standard_normal(512).astype(np.float32)
    n = f.astype(np.float64) / np.linalg.norm(f.astype(np.float64), axis=1, keepdims=True)
    m = n @ n.T
    np.fill_diagonal(m, 0)
    cf, ct = scores(torch.from_numpy(f).to(dev), torch.from_numpy(t).to(dev))
    assert abs(cf - m.sum() / (37 * 36)) < 1e-12 and abs(ct - float((n @ (t / np.linalg.norm(t.astype(np.float64)))).mean())) < 1e-12
    assert scores(torch.from_numpy(f).to(dev))[1] is None


def test_metric_is_deterministic(dev, engine, G):
    """Two runs of the whole metric (preprocess, encoder, scores) give identical bits."""
    from tc_light_amd.evaluate import clip_frame, clip_text
    frames = torch.from_numpy(G["frames"])
    with pytest.warns(UserWarning):
        a = (clip_frame(frames, engine), clip_text(frames, "soft warm light. from the left", engine, None, allow_random=True))
        b = (clip_frame(frames, engine), clip_text(frames, "soft warm light. from the left", engine, None, allow_random=True))
    assert a == b
    assert torch.equal(engine.encode_image(frames), engine.encode_image(frames))


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_evaluate_cli_with_clip(dev, tmp_path):
    """evaluate.py --clip <absent file> with random weights allowed: result.txt carries clip-frame, clip-text and warp-error-ssim (+ z_*) in sorted
    order, the two prompts' blocks differ in clip-text, and only pick-score is named as not computed."""
    import yaml
    from tc_light_amd.dataparser import write_mjpeg_avi
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (1, 150, 220, 3), dtype=np.uint8)
    src = np.stack([np.roll(base[0], (k, 2 * k), (0, 1)) for k in range(4)])
    edit = np.clip(src[:, 5:135, 7:205].astype(np.int32) + 20, 0, 255).astype(np.uint8)
    write_mjpeg_avi(str(tmp_path / "output.avi"), edit)
    write_mjpeg_avi(str(tmp_path / "output_gt.avi"), src)
    cfg = {"generation": {"prompt": {"a": "soft light", "b": "warm light from the left window"}}, "models": {"raft": str(tmp_path / "absent.pth")},
           "sec_per_frame": 0.5, "max_memory_allocated": 1000.0, "total_number_of_frames": 4, "total_time": 2.0}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, TCL_ALLOW_RANDOM_WEIGHTS="1")
    r = subprocess.run(["timeout", "-k", "10", "140", sys.executable, os.path.join(ROOT, "evaluate.py"), "--output_dir", str(tmp_path), "--eval_cost",
                        "--clip", str(tmp_path / "absent_clip.pt")], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    note = [ln for ln in r.stdout.splitlines() if "not computed here" in ln]
    assert len(note) == 1 and "pick-score" in note[0] and "clip-frame" not in note[0] and "clip-text" not in note[0]
    lines = (tmp_path / "result.txt").read_text().splitlines()
    assert lines[0] == "unknown_video - warm light from the left window"
    keys = [ln.split(": ")[0] for ln in lines[1:]]
    assert keys == ["clip-frame", "clip-text", "warp-error-ssim", "z_fps", "z_max_memory_allocated(M)", "z_resolution", "z_total_frames", "z_total_time(s)"]
    blocks = r.stdout.split("unknown_video - ")[1:]
    assert len(blocks) == 2
    vals = [dict(ln.split(": ") for ln in b.splitlines()[1:] if ": " in ln) for b in blocks]
    assert vals[0]["clip-frame"] == vals[1]["clip-frame"] and vals[0]["warp-error-ssim"] == vals[1]["warp-error-ssim"]
    assert vals[0]["clip-text"] != vals[1]["clip-text"]
    assert all(len(v["clip-text"].split(".")[1]) == 4 and -1.0 <= float(v["clip-text"]) <= 1.0 for v in vals)
