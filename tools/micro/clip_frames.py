"""The CLIP leg of evaluate.py at 1280x720: preprocess (tcl_clip_preprocess_u8), the ViT-B/32 image encoder and the scores kernel for a 300-frame clip
(device events after a warm-up at the same shapes), then clip_frame + clip_text as evaluate.py calls them (host clock around a synchronise).  Seeded
stand-in weights.  Prints one JSON line.   python tools/micro/clip_frames.py [--json out.json] [--frames N] [--batch B]"""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tc_light_amd import clip as C  # noqa: E402
from tc_light_amd.evaluate import clip_frame, clip_text  # noqa: E402

H, W = 720, 1280


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def events(fn, n):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n


def main():
    n, batch = arg("--frames", 300), arg("--batch", 64)
    g = torch.Generator().manual_seed(0)
    eng = C.CLIPEngine(C.seeded_state_dict(6), "cuda")
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    res = dict(shape=[H, W], frames=n, batch=batch)

    def pre():
        for s in range(0, n, batch):
            eng.preprocess(frames[s:s + batch])

    t = events(pre, 3)
    res.update(preprocess_s=t, preprocess_us_per_frame=t / n * 1e6, preprocess_read_gbs=n * H * W * 3 / t / 1e9)
    chunks = [eng.preprocess(frames[s:s + batch])[0] for s in range(0, n, batch)]

    def enc():
        return [eng.encode_patches(p, p.shape[0] // eng.grid ** 2) for p in chunks]

    t = events(enc, 3)
    flops = C.useful_flops(eng, n)
    res.update(encoder_s=t, encoder_ms_per_frame=t / n * 1e3, encoder_gflop_per_image=flops / n / 1e9, encoder_tflops=flops / t / 1e12)
    feats = torch.cat(enc())
    text = eng.encode_text(C.tokenize("a b c", None, allow_random=True))[0]
    t = events(lambda: C.scores(feats, text), 10)
    res.update(scores_s=t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cf = clip_frame(frames, eng, batch=batch)
    ct = clip_text(frames, "soft warm light from the left", eng, None, allow_random=True, batch=batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res.update(clip_frame_plus_clip_text_s=dt, clip_frame=cf, clip_text=ct)
    print(f"{n} frames {W}x{H}: preprocess {res['preprocess_s'] * 1e3:.1f} ms ({res['preprocess_read_gbs']:.0f} GB/s read), encoder "
          f"{res['encoder_s'] * 1e3:.1f} ms ({res['encoder_tflops']:.1f} TFLOP/s), scores {res['scores_s'] * 1e3:.2f} ms; clip_frame + clip_text as "
          f"evaluate.py calls them (the frames encoded twice) {dt:.2f} s")
    print(json.dumps(res))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    main()
