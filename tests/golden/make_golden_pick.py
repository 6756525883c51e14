"""Golden vectors for pick-score: `transformers.CLIPModel` at the full PickScore_v1 architecture (CLIP ViT-H/14: 32 + 24 layers, 16 heads per tower,
erf GELU; tc_light_amd.clip.PICKSCORE_V1), loaded with the seeded stand-in weights of tc_light_amd.clip through to_hf_state (strict=True) and run in
f32 on the CPU over frames preprocessed by `CLIPImageProcessorPil` (shortest edge 224, bicubic, centre crop 224, CLIP mean / std: the processor of
laion/CLIP-ViT-H-14-laion2B-s32B-b79K, the one pick_score_func is fed by; the torchvision-backed processor is not the reference's and is not used).
Run from the repo root:   python tests/golden/make_golden_pick.py   (a few minutes and about 20 GB on 8 cores; writes pick.npz, which holds no weights:
the tests regenerate them from the seed).

Stored: the uint8 frames of two short clips (clip A at 227 x 224, a size at which transformers' floor crop and clip's rounded crop differ by a row;
clip B at 180 x 240), the raw token ids of two prompts (the second has 90, so the processor's truncation to 75 is exercised), the f32 image and text
features, the per-image and mean scores exp(logit_scale) cos(text, image) in f64, and the f16 floor: the same model with .half() on the CPU (every
op's output rounded to f16) against its f32 self, features and rel-L2.  The script asserts that the two clips' pick-scores differ by at least ten
times the tolerance the GPU test applies, exp(logit_scale) (2 floor_image + 2 floor_text), for the prompt the clips were chosen by: otherwise the test could not see a wrong encoder."""
import math
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
from tc_light_amd import clip as C  # noqa: E402

SEED = 7
N_RAW = (9, 90)                         # raw token counts of the two prompts


class StoredIds:
    """The tokenizer interface tokenize_truncated reads, answering with a stored id list (the golden's prompts are id lists, not text)."""
    bos_token_id, eos_token_id = C.SOT, C.EOT

    def __init__(self, ids):
        self.ids = [int(i) for i in ids]

    def __call__(self, text, **kw):
        return {"input_ids": list(self.ids)}


def smooth_field(g, H, W, cells):
    small = (g.random((cells, cells, 3)) * 255).astype(np.uint8)
    return np.asarray(Image.fromarray(small).resize((W, H), Image.BILINEAR))


def candidates(H, W, seed=0, n=10):
    """A pool of unlike uint8 frames: smooth colour fields of several grain sizes."""
    g = np.random.default_rng(seed)
    return np.stack([smooth_field(g, H, W, (2, 3, 5, 9, 17)[i % 5]) for i in range(n)])


def pixel_values(processor, frames):
    return processor(images=[Image.fromarray(f) for f in frames], return_tensors="pt")["pixel_values"]


def features(model, px, rows):
    with torch.no_grad():
        v = model.visual_projection(model.vision_model(pixel_values=px).pooler_output)
        t = torch.cat([model.text_projection(model.text_model(input_ids=r).pooler_output) for r in rows])
    return v.float(), t.float()


def pick(v, t, logit_scale):
    """pick_score_func (eval_utils.py:163-176) in f64: per-image scores and their mean."""
    s = math.exp(logit_scale) * (torch.nn.functional.normalize(v.double(), dim=-1) @ torch.nn.functional.normalize(t.double(), dim=-1))
    return s.numpy(), float(s.mean())


def main():
    from transformers import CLIPConfig, CLIPModel
    from transformers.models.clip import CLIPImageProcessorPil
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    A = C.PICKSCORE_V1
    model = CLIPModel(CLIPConfig(**C.to_hf_config(A))).eval()
    vc = model.config.vision_config
    assert (vc.hidden_act, vc.patch_size, vc.num_attention_heads, vc.num_hidden_layers, model.config.text_config.num_hidden_layers) == ("gelu", 14, 16, 32, 24)
    sd = C.seeded_state_dict(SEED, **C.arch_shapes(A))
    logit_scale = float(sd["logit_scale"])
    model.load_state_dict(C.to_hf_state(sd), strict=True)
    del sd
    processor = CLIPImageProcessorPil(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, resample=Image.BICUBIC)

    g = np.random.default_rng(1)
    raw = [g.integers(1000, 40000, n).tolist() for n in N_RAW]
    rows = [torch.tensor([[C.SOT] + r[:75] + [C.EOT]]) for r in raw]
    for r, row in zip(raw, rows):
        assert torch.equal(C.tokenize_truncated("", StoredIds(r)), row)
    assert rows[1].shape[1] == 77 and rows[0].shape[1] == N_RAW[0] + 2

    # choose inputs, not results: from a pool, the base of the near-static clip A is the frame closest to prompt 0 and clip B is the three farthest
    pool = candidates(180, 240)
    pv, pt = features(model, pixel_values(processor, pool), rows)
    cos_t = (torch.nn.functional.normalize(pv.double(), dim=-1) @ torch.nn.functional.normalize(pt[0].double(), dim=-1)).numpy()
    pn = torch.nn.functional.normalize(pv.double(), dim=-1)
    print("pool: cosines to prompt 0:", cos_t.round(3))
    print("pool: cosines between frames:\n", (pn @ pn.t()).numpy().round(2))
    order = np.argsort(cos_t)
    base = np.asarray(Image.fromarray(pool[order[-1]]).resize((224, 227), Image.BILINEAR))                 # 227 rows x 224 columns
    clip_a = np.stack([np.clip(base.astype(np.int16) + g.integers(-2, 3, base.shape), 0, 255).astype(np.uint8) for _ in range(3)])
    clip_b = pool[order[:3]]
    assert C.resize_geometry_rule(227, 224, 224, "floor") != C.resize_geometry_rule(227, 224, 224, "round")

    px = [pixel_values(processor, c) for c in (clip_a, clip_b)]
    pxs = torch.cat(px)
    v, t = features(model, pxs, rows)
    v16, t16 = features(model.half(), pxs.half(), rows)
    model.float()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    floor_img, floor_txt = rel(v16, v), rel(t16, t)
    na = len(clip_a)
    out = dict(seed=np.int64(SEED), logit_scale=np.float64(logit_scale), frames_a=clip_a, frames_b=clip_b, raw_ids_0=np.array(raw[0], dtype=np.int64),
               raw_ids_1=np.array(raw[1], dtype=np.int64), image_features=v.numpy(), text_features=t.numpy(), image_features_f16=v16.numpy(),
               text_features_f16=t16.numpy(), f16_floor_image=np.float64(floor_img), f16_floor_text=np.float64(floor_txt))
    per, mean = {}, np.zeros((2, 2))
    for p in range(2):
        for c, sl in enumerate((slice(0, na), slice(na, None))):
            per[p, c], mean[p, c] = pick(v[sl], t[p], logit_scale)
    out["scores"] = np.stack([np.concatenate([per[p, 0], per[p, 1]]) for p in range(2)])                   # [prompt, image]
    out["pick_score"] = mean                                                                               # [prompt, clip]
    tol = math.exp(logit_scale) * (2 * floor_img + 2 * floor_txt)
    print(f"f16 floor: image {floor_img:.3e}, text {floor_txt:.3e} -> score tolerance {tol:.3e}")
    print("pick-score [prompt, clip]:\n", mean)
    print("per-image scores [prompt, image]:\n", out["scores"].round(3))
    assert abs(mean[0, 0] - mean[0, 1]) >= 10 * tol, "pick-score (prompt 0, the one the clips were chosen by) does not separate the two clips"
    path = os.path.join(ROOT, "tests", "golden", "pick.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
