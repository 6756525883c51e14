"""GPU: the UNet engine really runs LoRA-merged weights (`load_unet_state(..., lora=...)`, tc_light_amd/lora.py) and start latents from
`generation.latents_path` really start the denoising loop.

Parity: the engine is loaded through the loader with seeded weights and the LoRA set of
tests/lora_sets.py; the oracle UNet gets a state dict merged independently here (float64 product, cast to f32).  One `forward_many` on the smallest
case of tests/test_gpu_unet.py::test_unet_small_odd_planes_vs_oracle -- a 4x8 latent, chunks [2, 4, 2], 77 text tokens, VidToMe off -- under that
test's tolerance for the shape, rel-L2 < 1e-2 per chunk: merged weights are just other weights.
Really applied: the factors are sized like the seeded weights themselves (lora_sets.factors: up @ down ~ 1/sqrt(fan_in)), so that the oracle with and
without the LoRA differ by >= 10x that tolerance (asserted on the CPU oracle: >= 0.1; it is ~1, a random network decorrelates); the engine must
be within the tolerance of the LoRA oracle and outside it from the base oracle.  On a loader that ignores
`lora` the engine reproduces the base oracle and this fails.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import lora_sets as S

pytestmark = pytest.mark.gpu

TOL = 1e-2                      # tests/test_gpu_unet.py::test_unet_small_odd_planes_vs_oracle
WEIGHT = 0.8
HH, WW, FS, LT, T = 4, 8, [2, 4, 2], 77, 501.0


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import sd15 as OS
    from tc_light_amd import model_utils, sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    fs = S.factors()
    block = {"pretrained_model_name_or_path_or_dict": S.kohya(fs), "lora_weight_name": None, "lora_adapter": None, "lora_weight": WEIGHT}
    # the loader is called twice (without and with the LoRA); drawing the 860 M seeded stand-in values takes ~20 s on the host and is deterministic, so the
    # second call gets a copy of the first call's tensors
    draw, drawn = sd15.random_state_dict, {}

    def draw_once(shapes, seed, gain=1.0):
        if (seed, gain) not in drawn:
            drawn[(seed, gain)] = draw(shapes, seed, gain)
        return {k: v.clone() for k, v in drawn[(seed, gain)].items()}
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
        mp.setattr(sd15, "random_state_dict", draw_once)
        warnings.simplefilter("ignore")                     # seeded stand-in weights are asked for on purpose
        base = model_utils.load_unet_state(None, None, seed=1, allow=True)
        merged = model_utils.load_unet_state(None, None, seed=1, allow=True, lora=block)
    own = dict(base)
    own.update({k: v.float() for k, v in S.merged64(base, fs, WEIGHT).items()})          # the independent merge
    eng = UNetEngine(merged, "cuda", VidToMe("cuda", seed=5, enabled=False))
    F = sum(FS)
    g = np.random.default_rng(40 + HH)
    x = torch.from_numpy(g.standard_normal((F, 8, HH, WW)).astype(np.float32)).half().float()
    text = torch.from_numpy(np.random.default_rng(HH).standard_normal((2, LT, 768)).astype(np.float32)).half().float()
    xin = torch.cat([x, x]).permute(0, 2, 3, 1).contiguous().cuda().half()
    eps = eng.forward_many(xin, FS, HH, WW, T, text.cuda().half()).view(2 * F, HH, WW, 4).permute(0, 3, 1, 2).float().cpu()
    torch.cuda.synchronize()
    # VidToMe is off, so the samples are independent: one oracle call over all chunks, sliced per chunk below
    with torch.no_grad():
        ref_lora = OS.unet_forward(own, torch.cat([x, x]), T, text)
        ref_base = OS.unet_forward(base, torch.cat([x, x]), T, text)
    return dict(eng=eng, eps=eps, ref_lora=ref_lora, ref_base=ref_base, base=base, merged=merged, own=own, fs=fs)


def _chunks(t):
    F, off = sum(FS), 0
    for f in FS:
        yield torch.cat([t[off:off + f], t[F + off:F + off + f]])
        off += f


def test_engine_on_loader_merged_weights_equals_oracle_on_independent_merge(setup):
    assert torch.isfinite(setup["eps"]).all()
    touched = {p + ".weight" for p, *_ in setup["fs"]}
    for k, v in setup["own"].items():                                                     # the loader's merge is the independent one to f32 rounding
        if k not in touched:
            assert torch.equal(setup["merged"][k], setup["base"][k]), k
        else:
            assert float((setup["merged"][k] - v).abs().max()) <= 1e-6 * float(v.abs().max()), k
    for i, (got, ref) in enumerate(zip(_chunks(setup["eps"]), _chunks(setup["ref_lora"]))):
        r = rel(got, ref)
        print(f"[lora parity] chunk {i} ({FS[i]} frames): engine vs f32 oracle on merged weights rel-L2 = {r:.3e}")
        assert r < TOL, (i, r)


def test_lora_is_really_applied(setup):
    gap = rel(setup["ref_lora"], setup["ref_base"])
    r_lora, r_base = rel(setup["eps"], setup["ref_lora"]), rel(setup["eps"], setup["ref_base"])
    print(f"[lora applied] oracle with vs without the LoRA rel-L2 = {gap:.3e}; engine vs LoRA oracle {r_lora:.3e}, vs base oracle {r_base:.3e}")
    assert gap >= 10 * TOL, gap                              # CPU oracle alone: the seeded LoRA moves the output well clear of the tolerance
    assert r_lora < TOL and r_base > TOL, (r_lora, r_base)


def test_start_latents_from_file_drive_the_first_step(setup, tmp_path):
    """prepare_data with a latents file present: init_noise is the file's tensor (selected frames) in f16, and one denoise step from it is, bit
    for bit, one step from the same tensor put there by hand (the kernels are deterministic, VidToMe is off)."""
    from tc_light_amd import dataparser as D
    from tc_light_amd.generate import Generator
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    eng = setup["eng"]
    n, ids = 3, [0, 2, 3]
    cfg = dict(n_timesteps=1, alpha_t=0.0, chunk_size=4, guidance_scale=2.0, seed=77, noise_mode="same")
    sch = DPMSolverSDEScheduler()
    sch.set_timesteps(1)
    d = D.get_latents_dir(str(tmp_path), "iclight")
    os.makedirs(d)
    gen = torch.Generator().manual_seed(3)
    saved = torch.randn(5, 4, HH, WW, generator=gen)
    torch.save(saved, D.latent_file(d, sch.timesteps[0]))
    conds = torch.randn(2, 77, 768, generator=gen).half().cuda()
    cc = torch.randn(n, 4, HH, WW, generator=gen).half().cuda()
    frames = torch.zeros(n, 3, 8 * HH, 8 * WW, device="cuda")

    def one_step(g, x0):
        x = g.ddim_sample(x0.clone(), conds, conds, cc)
        torch.cuda.synchronize()
        return x.clone()
    ga = Generator(eng, None, dict(cfg, latents_path=str(tmp_path), model_key="iclight", frame_ids=ids))
    ga.prepare_data(frames)
    want = saved[ids].to(torch.float16)
    assert ga.init_noise.dtype == torch.float16 and ga.init_noise.is_cuda and torch.equal(ga.init_noise.cpu(), want)
    xa = one_step(ga, ga.init_noise)
    gb = Generator(eng, None, cfg)                           # no latents_path: draws its own noise ...
    gb.prepare_data(frames)
    assert not torch.equal(gb.init_noise.cpu(), want)
    x_own = one_step(gb, gb.init_noise)
    gb.prepare_data(frames)
    xb = one_step(gb, want.cuda())                          # ... and the file's tensor injected by hand
    assert torch.isfinite(xa.float()).all() and torch.equal(xa, xb) and not torch.equal(xa, x_own)
