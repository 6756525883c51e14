"""RAFT rate at 1280x720 (seeded weights, 20 iterations): one pair through RAFTEngine.forward, then estimate_flows_raft on 16 frames at batch 1, 2
and 4 (fnet / cnet once per frame, 30 pairs).  Prints ms per pair and TFLOP/s on the useful-FLOP count of raft.useful_flops (the reference's
work per pair: three encoder passes, 20 update blocks with the context term folded, the mask head once).
python tools/micro/raft_pair.py [--json out.json] [--driver BATCH: one driver pass only, for rocprofv3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tc_light_amd.raft import RAFTEngine, estimate_flows_raft, seeded_state_dict, useful_flops  # noqa: E402

PEAK = 2.5e15                                                          # MI355X dense f16 MFMA peak, FLOP/s


def timed(fn, n):
    fn(); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def main():
    H, W = 720, 1280
    eng = RAFTEngine(seeded_state_dict(5), "cuda")
    if "--driver" in sys.argv:                                         # one pass of the driver alone (for a kernel trace): 16 frames at this batch
        bs = int(sys.argv[sys.argv.index("--driver") + 1])
        frames = torch.rand(16, 3, H, W, generator=torch.Generator().manual_seed(0)).cuda()
        estimate_flows_raft(eng, frames, batch=bs); torch.cuda.synchronize()
        return
    fl = useful_flops(H, W)
    g = torch.Generator().manual_seed(0)
    a = (torch.rand(1, 3, H, W, generator=g) * 255).cuda()
    b = torch.roll(a, (3, 5), (2, 3))
    res = dict(shape=[H, W], iters=20, useful_tflop_per_pair=fl["total"] / 1e12, flop_breakdown_g={k: v / 1e9 for k, v in fl.items()})
    s = timed(lambda: eng.forward(a, b, iters=20), 5)
    res["forward_ms_per_pair"] = s * 1e3
    res["forward_tflops"] = fl["total"] / s / 1e12
    print(f"forward 1 pair: {s * 1e3:.2f} ms  {fl['total'] / s / 1e12:.1f} TFLOP/s  ({fl['total'] / s / PEAK * 100:.1f} % of 2.5 PF)")
    frames = torch.rand(16, 3, H, W, generator=g).cuda()
    npairs = 2 * (16 - 1)
    for bs in (1, 2, 4):
        s = timed(lambda: estimate_flows_raft(eng, frames, batch=bs), 2)
        per = s / npairs
        res[f"driver_b{bs}_ms_per_pair"] = per * 1e3
        res[f"driver_b{bs}_tflops"] = fl["total"] / per / 1e12
        print(f"estimate_flows_raft 16 frames batch {bs}: {s * 1e3:.1f} ms, {per * 1e3:.2f} ms/pair, {fl['total'] / per / 1e12:.1f} TFLOP/s (reference work)")
    print(json.dumps(res))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
