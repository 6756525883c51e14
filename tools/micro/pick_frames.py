"""The pick-score leg of evaluate.py at 1280x720: preprocess (tcl_clip_preprocess_ld_u8, floor crop, 640-column patch rows), the ViT-H/14 image tower
of PickScore_v1 and one prompt (text tower + tcl_pick_scores) for a 300-frame clip.  Device events after a warm-up at the same shapes, several
repeats (median and spread), the attention kernel alone at the tower's shape, and a plain f16 GEMM of the MLP's shape through tcl_gemm_f16 as the
box's own yardstick beside them.  Seeded stand-in weights.  Prints one JSON line.
python tools/micro/pick_frames.py [--json out.json] [--frames N] [--batch B] [--repeats R]"""
import json
import math
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tc_light_amd import clip as C  # noqa: E402
from tc_light_amd.lib import lib, stream  # noqa: E402

H, W = 720, 1280


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def events(fn, repeats):
    """Seconds of fn per repeat (device events), after one warm-up call."""
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 1e3)
    return out


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def main():
    n, batch, rep = arg("--frames", 300), arg("--batch", 64), arg("--repeats", 5)
    g = torch.Generator().manual_seed(0)
    eng = C.pick_engine(C.seeded_state_dict(7, **C.arch_shapes(C.PICKSCORE_V1)), "cuda")
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    res = dict(shape=[H, W], frames=n, batch=batch, repeats=rep)

    def pre():
        for s in range(0, n, batch):
            eng.preprocess(frames[s:s + batch])

    t = summary(events(pre, rep))
    res.update(preprocess_s=t, preprocess_read_gbs=n * H * W * 3 / t["median"] / 1e9)
    chunks = [eng.preprocess(frames[s:s + batch])[0] for s in range(0, n, batch)]

    def enc():
        return [eng.encode_patches(p, p.shape[0] // eng.grid ** 2) for p in chunks]

    t = summary(events(enc, rep))
    flops = C.useful_flops(eng, n)
    res.update(encoder_s=t, encoder_ms_per_frame=t["median"] / n * 1e3, encoder_gflop_per_image=flops / n / 1e9, encoder_tflops=flops / t["median"] / 1e12)
    feats = torch.cat(enc())
    ids = C.tokenize_truncated("soft warm light from the left window", None, allow_random=True)
    t = summary(events(lambda: C.pick_scores(feats, eng.encode_text(ids)[0], eng.logit_scale), rep))
    res.update(prompt_s=t)

    # the attention kernel alone at the tower's shape: one batch of 64 images, 16 heads, T = 257, d = 80; all layers of all batches = layers * n / batch calls
    T, heads, d = eng.grid ** 2 + 1, eng.visual.heads, eng.vwidth // eng.visual.heads
    qkv = torch.randn(batch * T, 3 * eng.vwidth, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").half()
    ta = summary(events(lambda: eng.attention(qkv, batch, T, heads, False), 20))
    calls = len(eng.visual.layers) * n / batch
    res.update(attention_call_s=ta, attention_tflops=4 * batch * T * T * eng.vwidth / ta["median"] / 1e12,
               attention_share_of_encoder=ta["median"] * calls / res["encoder_s"]["median"])

    # yardstick: the MLP's c_fc GEMM alone (M = batch * 257, N = 5120, K = 1280) on this box, now
    M, N, K = batch * T, 4 * eng.vwidth, eng.vwidth
    a = torch.randn(M, K, device="cuda").half(); w = torch.randn(N, K, device="cuda").half(); y = torch.empty(M, N, dtype=torch.float16, device="cuda")
    tg = summary(events(lambda: lib().tcl_gemm_f16(a, w, 0, 0, y, M, N, K, K, K, N, N, 0, stream()), 20))
    res.update(gemm_alone_shape=[M, N, K], gemm_alone_s=tg, gemm_alone_tflops=2 * M * N * K / tg["median"] / 1e12)
    tg4 = summary(events(lambda: lib().tcl_gemm_f16(a, w, 0, 0, y, M, N, K, K, K, N, N, 4, stream()), 20))
    res.update(gemm_gelu_alone_tflops=2 * M * N * K / tg4["median"] / 1e12)

    print(f"{n} frames {W}x{H}: preprocess {res['preprocess_s']['median'] * 1e3:.1f} ms ({res['preprocess_read_gbs']:.0f} GB/s read), image tower "
          f"{res['encoder_s']['median']:.3f} s ({res['encoder_tflops']:.0f} TFLOP/s useful; min {res['encoder_s']['min']:.3f} max {res['encoder_s']['max']:.3f}), "
          f"one prompt {res['prompt_s']['median'] * 1e3:.1f} ms; attention {ta['median'] * 1e3:.2f} ms per call = {res['attention_share_of_encoder'] * 100:.1f} % "
          f"of the tower; c_fc GEMM alone {res['gemm_alone_tflops']:.0f} TFLOP/s ({res['gemm_gelu_alone_tflops']:.0f} with the GELU epilogue)")
    print(json.dumps(res))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    main()
