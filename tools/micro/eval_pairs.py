"""warp-error-ssim rates at 1280x720: the warp + mask kernel and the SSIM kernel per frame pair (batches of 4 pairs, device events), then the whole
`warp_ssim` (RAFT flows with seeded weights + the two kernels) on a synthetic 300-frame clip.  Prints one JSON line.
python tools/micro/eval_pairs.py [--json out.json] [--frames N]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tc_light_amd.evaluate import ssim_u8, warp_mask_planes, warp_ssim, warp_ssim_from_flows  # noqa: E402
from tc_light_amd.raft import RAFTEngine, seeded_state_dict  # noqa: E402

H, W, B = 720, 1280, 4
HBM = 8.0e12                                                           # MI355X HBM3E peak, bytes/s


def events(fn, n):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n


def clip(n, g):
    """n frames of one random texture translated by (k, 2k) px: uint8 [n,H,W,3] on the device (source) and a brightened copy (edit)."""
    base = torch.randint(0, 256, (H + 2 * n, W + 4 * n, 3), generator=g, dtype=torch.uint8).cuda()
    base = torch.nn.functional.avg_pool2d(base.permute(2, 0, 1)[None].float(), 5, 1, 2)[0].permute(1, 2, 0).to(torch.uint8)
    src = torch.stack([base[k:k + H, 2 * k:2 * k + W] for k in range(n)]).contiguous()
    return src, (src.int() + 12).clamp(0, 255).to(torch.uint8)


def main():
    nframes = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else 300
    g = torch.Generator().manual_seed(0)
    res = dict(shape=[H, W], batch=B)
    edit = torch.randint(0, 256, (B + 1, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    byt = 2 * 2 * H * W * 4 + 2 * H * W * 3 + 2 * H * W * 3            # fwd + bwd planes, two edit frames, the two u8 planes written
    # smooth flows (a video's: neighbouring pixels gather neighbouring taps) and incoherent ones (independent per pixel, 3 px standard deviation)
    smooth = torch.nn.functional.interpolate(6 * torch.randn(B + 1, 2, H // 32, W // 32, generator=g), size=(H, W), mode="bilinear")
    for kind, f in (("smooth", smooth + 0.1 * torch.randn(B + 1, 2, H, W, generator=g)), ("incoherent", 3 * torch.randn(B + 1, 2, H, W, generator=g))):
        fut = f.cuda()
        past = -fut.roll(1, 0) + 0.1 * torch.randn(B + 1, 2, H, W, generator=g).cuda()
        s = events(lambda: warp_mask_planes(edit, fut, past, 0, B), 50) / B
        res.update({f"warp_mask_{kind}_us_per_pair": s * 1e6, f"warp_mask_{kind}_gbs": byt / s / 1e9})
    res["warp_mask_hbm_floor_us"] = byt / HBM * 1e6
    w, t = warp_mask_planes(edit, fut, past, 0, B)
    s = events(lambda: ssim_u8(w, t), 50) / B
    byt = 2 * H * W * 3
    res.update(ssim_us_per_pair=s * 1e6, ssim_gbs=byt / s / 1e9, ssim_hbm_floor_us=byt / HBM * 1e6)
    s = events(lambda: warp_ssim_from_flows(edit, fut, past, batch=B), 20) / B
    res["metric_from_flows_us_per_pair"] = s * 1e6
    print(f"per 1280x720 pair: warp+mask {res['warp_mask_smooth_us_per_pair']:.1f} us smooth ({res['warp_mask_smooth_gbs']:.0f} GB/s), "
          f"{res['warp_mask_incoherent_us_per_pair']:.1f} us incoherent flows, "
          f"ssim {res['ssim_us_per_pair']:.1f} us ({res['ssim_gbs']:.0f} GB/s), warp_ssim_from_flows {s * 1e6:.1f} us")
    eng = RAFTEngine(seeded_state_dict(5), "cuda")
    src, ed = clip(8, g)
    warp_ssim(ed, src, eng, batch=B); torch.cuda.synchronize()        # warm-up at the same size
    del src, ed
    src, ed = clip(nframes, g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score, per = warp_ssim(ed, src, eng, batch=B)
    dt = time.perf_counter() - t0
    res.update(frames=nframes, warp_ssim_s=dt, warp_ssim_ms_per_pair=dt / (nframes - 1) * 1e3, warp_ssim_score=score)
    print(f"warp_ssim on {nframes} frames: {dt:.2f} s ({dt / (nframes - 1) * 1e3:.2f} ms per pair), score {score:.6f}")
    print(json.dumps(res))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
