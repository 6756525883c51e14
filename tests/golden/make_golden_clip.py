"""Golden vectors for the CLIP figures (clip-frame / clip-text): `transformers.CLIPModel` at ViT-B/32 size (quick_gelu, the architecture of OpenAI's
clip.load("ViT-B/32")), loaded with the seeded stand-in weights of tc_light_amd.clip through to_hf_state (strict=True) and run in f32 on the CPU over
frames preprocessed with PIL (resize BICUBIC to short side 224, centre crop, / 255, normalise).  Run from the repo root:
python tests/golden/make_golden_clip.py   (writes clip.npz; the weights are regenerated from the seed by the tests).

Stored: the uint8 frames of two short clips (one nearly static, one whose frames differ strongly), two token-id rows, the f32 image and text features,
clip-frame and clip-text of both clips (sklearn's / torch's formulas restated in f64), and the f16 floor: the same model with .half() on the CPU
against its f32 self (rel-L2 of the features).  The script asserts that each figure differs between the two clips by at least 100 times the
tolerance the GPU test applies to it (4 x the floor): otherwise the test could not see a wrong encoder."""
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
from tc_light_amd import clip as C  # noqa: E402

SEED = 6
MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)


def pil_crop(frame, side=224):
    """clip's _transform up to the uint8 image: Resize(side, BICUBIC) + CenterCrop(side) on a PIL image."""
    H, W = frame.shape[:2]
    oh, ow, top, left = C.resize_geometry(H, W, side)
    im = Image.fromarray(frame).resize((ow, oh), Image.BICUBIC)
    return np.asarray(im)[top:top + side, left:left + side]


def pixel_values(frames):
    x = torch.from_numpy(np.stack([pil_crop(f) for f in frames])).permute(0, 3, 1, 2).float().div(255)
    return (x - MEAN) / STD


def smooth_field(g, H, W, cells):
    """A smooth random colour image: a cells x cells x 3 grid of uniform colours up-sampled bilinearly."""
    small = (g.random((cells, cells, 3)) * 255).astype(np.uint8)
    return np.asarray(Image.fromarray(small).resize((W, H), Image.BILINEAR))


def candidates(seed=0, n=24, H=180, W=240):
    """A pool of unlike uint8 frames: smooth colour fields of several grain sizes, some with strong noise on top."""
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        f = smooth_field(g, H, W, (2, 3, 5, 9, 17, 33)[i % 6]).astype(np.int16)
        if i % 4 == 3:
            f = f + g.integers(-60, 61, f.shape)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return np.stack(out)


def pick_clips(cos, cos_t, n=4):
    """From the pool's cosine matrix and its cosines to text row 0: the base frame of the static clip and the n frames of the varying clip that
    maximise min(1 - clip-frame(varying), |clip-text(static) - clip-text(varying)|).  Choosing inputs, not results: the figures are then computed from
    the chosen frames by the reference model."""
    import itertools
    best = (-1.0, None, None)
    N = len(cos_t)
    for sub in itertools.combinations(range(N), n):
        idx = np.array(sub)
        cf = (cos[np.ix_(idx, idx)].sum() - n) / (n * (n - 1))
        ct = cos_t[idx].mean()
        rest = np.setdiff1d(np.arange(N), idx)
        s = rest[np.argmax(np.abs(cos_t[rest] - ct))]
        score = min(1 - cf, abs(cos_t[s] - ct))
        if score > best[0]:
            best = (score, int(s), idx)
    return best[1], best[2]


def features(model, px, ids):
    with torch.no_grad():
        v = model.visual_projection(model.vision_model(pixel_values=px).pooler_output)
        t = model.text_projection(model.text_model(input_ids=ids).pooler_output)
    return v, t


def clip_frame(f):
    f = f.double()
    n = f / f.norm(dim=-1, keepdim=True)
    m = n @ n.t()
    m.fill_diagonal_(0)
    return float(m.sum() / (len(f) * (len(f) - 1)))


def clip_text(f, t):
    return float(torch.cosine_similarity(t.double()[None], f.double()).mean())


def main():
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    model = CLIPModel(CLIPConfig()).eval()
    assert model.config.vision_config.hidden_act == "quick_gelu" and model.config.vision_config.patch_size == 32
    model.load_state_dict(C.to_hf_state(C.seeded_state_dict(SEED)), strict=True)

    ids = torch.zeros(2, 77, dtype=torch.int64)
    g = np.random.default_rng(1)
    for r, n in enumerate((7, 30)):
        ids[r, :n + 2] = torch.tensor([C.SOT] + g.integers(1000, 40000, n).tolist() + [C.EOT])
    pool = candidates()
    pv, pt = features(model, pixel_values(pool), ids)
    pn = torch.nn.functional.normalize(pv.double(), dim=-1)
    base, idx = pick_clips((pn @ pn.t()).numpy(), (pn @ torch.nn.functional.normalize(pt[0].double(), dim=-1)).numpy())
    static = np.stack([np.clip(pool[base].astype(np.int16) + g.integers(-2, 3, pool[base].shape), 0, 255).astype(np.uint8) for _ in range(4)])
    varying = pool[idx]
    frames = np.concatenate([static, varying])
    px = pixel_values(frames)
    v, t = features(model, px, ids)
    v16, t16 = features(model.half(), px.half(), ids)
    model.float()
    rel = lambda a, b: float((a.float() - b).norm() / b.norm())
    floor_img, floor_txt = rel(v16, v), rel(t16, t)
    ns = len(static)
    out = dict(seed=np.int64(SEED), frames=frames, n_static=np.int64(ns), ids=ids.numpy(), image_features=v.numpy(), text_features=t.numpy(),
               f16_floor_image=np.float64(floor_img), f16_floor_text=np.float64(floor_txt),
               clip_frame=np.array([clip_frame(v[:ns]), clip_frame(v[ns:])]),
               clip_text=np.array([[clip_text(v[:ns], t[r]), clip_text(v[ns:], t[r])] for r in range(2)]))
    floor = max(floor_img, floor_txt)
    tol = 4 * floor
    print(f"f16 floor: image {floor_img:.3e}, text {floor_txt:.3e} -> score tolerance {tol:.3e}")
    print("clip-frame (static, varying):", out["clip_frame"])
    print("clip-text per id row (static, varying):", out["clip_text"])
    cos = torch.nn.functional.normalize(v, dim=-1) @ torch.nn.functional.normalize(v, dim=-1).t()
    print("cosines between the varying frames:", cos[ns:, ns:].numpy().round(3))
    assert abs(out["clip_frame"][0] - out["clip_frame"][1]) >= 100 * tol, "clip-frame does not separate the two clips"
    assert abs(out["clip_text"][0, 0] - out["clip_text"][0, 1]) >= 100 * tol, "clip-text (id row 0) does not separate the two clips"
    path = os.path.join(ROOT, "tests", "golden", "clip.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
