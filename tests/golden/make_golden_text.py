"""Golden vectors for the prompt embeddings: `transformers.CLIPTextModel` at the size of SD-1.5's text encoder (tc_light_amd.clip.SD15_TEXT: the text
tower of CLIP ViT-L/14, quick_gelu), loaded with the seeded stand-in weights of tc_light_amd.clip.seeded_text_state_dict through to_hf_text_state
(strict=True; the `text_model.` prefix is dropped when the installed transformers' CLIPTextModel has no such level) and run in f32 on the CPU.
Run from the repo root:  python tests/golden/make_golden_text.py   (writes text.npz; the weights are regenerated from the seed by the tests).

Stored: three id rows in the layout of text.encode_prompt_inner ([BOS] + body + EOS up to 77) -- a short prompt (7 tokens), one that fills the 75
body cells exactly, and the ragged last chunk of the default negative prompt, which CLIP's vocabulary cuts into a few tokens more than 75 (4 here)
-- with random in-vocabulary ids; last_hidden_state [3, 77, 768] in f32; the seed; and f16_floor: the same model with .half() on the CPU against
its f32 self (rel-L2 over all rows), as make_golden_clip.py defines its floors."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
from tc_light_amd import clip as C  # noqa: E402

SEED = 8
BODIES = (7, 75, 4)


def main():
    from transformers import CLIPTextConfig, CLIPTextModel
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    A = C.SD15_TEXT
    model = CLIPTextModel(CLIPTextConfig(**C.to_hf_text_config(A))).eval()
    prefix = "text_model." if any(k.startswith("text_model.") for k in model.state_dict()) else ""
    model.load_state_dict(C.to_hf_text_state(C.seeded_text_state_dict(SEED, **A), prefix=prefix), strict=True)

    ids = torch.full((len(BODIES), A["context_length"]), C.EOT, dtype=torch.int64)
    ids[:, 0] = C.SOT
    g = np.random.default_rng(1)
    for r, n in enumerate(BODIES):
        ids[r, 1:1 + n] = torch.from_numpy(g.integers(1000, 40000, n))
    with torch.no_grad():
        h = model(input_ids=ids).last_hidden_state
        h16 = model.half()(input_ids=ids).last_hidden_state
    floor = float((h16.float() - h).norm() / h.norm())
    rows = ((h16.float() - h).norm(dim=-1) / h.norm(dim=-1))
    print(f"f16 floor (all rows) {floor:.3e}; per row: max {float(rows.max()):.3e}, median {float(rows.median()):.3e}")
    print("row norms: min %.3f max %.3f" % (float(h.norm(dim=-1).min()), float(h.norm(dim=-1).max())))
    # the rows differ from one another: an engine that mixed up positions or ids would be seen
    flat = torch.nn.functional.normalize(h.reshape(-1, h.shape[-1]).double(), dim=-1)
    print("largest cosine between two different rows of the short prompt's first 9: %.4f" % float((flat[:9] @ flat[:9].t()).fill_diagonal_(0).max()))
    out = dict(seed=np.int64(SEED), ids=ids.numpy(), last_hidden_state=h.numpy().astype(np.float32), f16_floor=np.float64(floor))
    path = os.path.join(ROOT, "tests", "golden", "text.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
