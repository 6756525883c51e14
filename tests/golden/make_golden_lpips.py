"""Writes tests/golden/lpips.npz: two short clips and the frame-lpips figures tests/lpips_refs.py gives for them, exact float64 and at the f16 floor,
with seeded stand-in weights (tc_light_amd.lpips.seeded_state: the file stores the generator's arguments, not the 15 M parameters).
    python tests/golden/make_golden_lpips.py
clip A: 4 relit and 4 source frames of 36 x 52 (padded to 40 x 56 by the metric).  clip B: the same relit frames against 4 source frames of
45 x 60, which the metric first resizes to 36 x 52 (PIL, default filter)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import torch  # noqa: E402

import lpips_refs as R  # noqa: E402
from tc_light_amd.evaluate import resize_like  # noqa: E402
from tc_light_amd.lpips import INPUT_SCALE  # noqa: E402

SEED, BIAS_STD = 8, 0.05


def _field(rng, n, h, w, cells):
    g = torch.from_numpy(rng.standard_normal((n, 3, cells, cells)))
    return torch.nn.functional.interpolate(g, size=(h, w), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).numpy()


def main():
    rng = np.random.default_rng(2024)
    n, h, w = 4, 36, 52
    base = 128 + 70 * _field(rng, n, 45, 60, 5) + 12 * rng.standard_normal((n, 45, 60, 3))
    source_b = np.clip(np.rint(base), 0, 255).astype(np.uint8)                              # 45 x 60
    source_a = resize_like(torch.from_numpy(source_b), h, w).numpy()                        # 36 x 52
    relit = source_a.astype(np.float64) * (0.8 + 0.3 * _field(rng, n, h, w, 3)) + 25 * _field(rng, n, h, w, 4) + 6 * rng.standard_normal((n, h, w, 3))
    edit = np.clip(np.rint(relit), 0, 255).astype(np.uint8)
    edit[:, 0, :, :] = 255                                                                  # borders far from the scaling layer's shift colour
    edit[:, :, -1, :] = 0
    source_a = source_a.copy()
    source_a[:, -1] = 240
    state = R.seeded_state(SEED, BIAS_STD)
    out = {"seed": np.int64(SEED), "bias_std": np.float64(BIAS_STD), "input_scale": np.float64(INPUT_SCALE), "edit": edit, "source_a": source_a,
           "source_b": source_b}
    for name, src in (("a", source_a), ("b", resize_like(torch.from_numpy(source_b), h, w).numpy())):
        for mode, f16 in (("exact", False), ("floor", True)):
            mean, per = R.frame_lpips(edit, src, state, s=INPUT_SCALE if f16 else 1.0, f16=f16)
            out[f"{name}_{mode}_mean"], out[f"{name}_{mode}_per"] = np.float64(mean), per
            print(name, mode, mean, per)
    np.savez_compressed(os.path.join(HERE, "lpips.npz"), **out)


if __name__ == "__main__":
    main()
