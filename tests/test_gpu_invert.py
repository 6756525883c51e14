"""GPU: DDIM inversion on the IC-Light UNet (tc_light_amd/invert.py, csrc/elem.hip: tcl_invert_pack_f16, tcl_ddim_step_f32).

1. Leaf, exact: the two kernels bit for bit against tests/invert_refs.py::ddim_step_ref and a numpy pack, both directions, frames and input records
   outside the group untouched, the inverse property within invert_refs.roundtrip_bound, the TCL_EINVAL cases.
2. Loop parity: the engine's 3-step inversion / reconstruction of 5 frames in two groups (4 + 1: the lone frame rides with its duplicate) against
   invert_ref / sample_ref over the f32 oracle, by rel-L2, with the f16 floor (the same loops over the oracle's f16-output mode) as the bar:
   engine <= 1.25 x floor, the margin test_gpu_unet.py's single forward uses.  Measured on an MI355X (profiles/invert_parity.txt): inversion 1.74e-3
   against a floor of 1.81e-3 (16x24) and 1.88e-3 against 2.01e-3 (10x14), reconstruction 2.78e-3 / 2.92e-3 and 2.86e-3 / 2.88e-3: ratios 0.93-0.99, so the
   margin was not widened.  One group against two groups: the same bits (with the GEMMs' K splits off, see there).  The oracle legs are twelve CPU UNet
   forwards per plane: about 10 s per case on 16 cores.
3. Producer meets consumer: Inverter.__call__ on a directory of PNGs -> Generator.prepare_data starts from rows frame_ids of the saved tensor.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import invert_refs as R

pytestmark = pytest.mark.gpu

STEPS, L_TEXT, N_FRAMES = 3, 77, 5
MARGIN = 1.25                                  # over the f16 floor; tests/test_gpu_unet.py::test_unet_two_chunks


def rel(a, b):
    return ((a.float().cpu() - b.float()).norm() / b.float().norm()).item()


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    sd = sd15.random_state_dict(sd15.unet_param_shapes(), seed=1)
    return sd, UNetEngine(sd, "cuda", VidToMe("cuda", seed=5))            # the generator's VidToMe: enabled, and it has to stay so


def _config(tmp, h, w, rgb_path=None, **inv):
    from tc_light_amd.config_utils import _wrap
    inversion = dict(save_path=os.path.join(str(tmp), "latents"), prompt="a street at dusk", n_frames=None, steps=STEPS, save_intermediate=False,
                     save_steps=STEPS, use_blip=False, recon=False, control="none", batch_size=64, force=False, max_tokens_per_pass=1 << 20)
    inversion.update(inv)
    return _wrap(dict(sd_version="iclight", model_key="iclight", seed=3, work_dir=str(tmp), data=dict(scene_type="video", rgb_path=rgb_path, height=8 * h, width=8 * w),
                      inversion=inversion, generation=dict(n_timesteps=STEPS, use_lora=False), models=dict(allow_random=True)))


def _inverter(eng, cfg, vae=None):
    from tc_light_amd.invert import Inverter
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    return Inverter(SimpleNamespace(unet=eng, vae=vae), DPMSolverSDEScheduler(), cfg)


# ---------------------------------------------------------------------------------------------------------------- 1. leaves
@pytest.mark.parametrize("h,w", [(5, 7), (16, 24)])
def test_pack_and_step_kernels_exact(h, w):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib, stream
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    L, dev = lib(), torch.device("cuda")
    g = np.random.default_rng(100 + h)
    N, F, Fv = 7, 6, 5
    idx_h = np.array([5, 2, 6, 0, 3, 3], np.int32)                       # a permutation of a strict subset (1 and 4 are absent) + the odd duplicate
    SENT = 77.0
    x0 = (g.standard_normal((N, 4, h, w)) * 2).astype(np.float32)
    cond = g.standard_normal((N, 4, h, w)).astype(np.float16)
    eps = g.standard_normal((F, h, w, 4)).astype(np.float16)
    sch = DPMSolverSDEScheduler()
    sch.set_timesteps(STEPS)
    ts = sorted(set(sch.timesteps.tolist()))
    idx, cond_d, eps_d = torch.from_numpy(idx_h).to(dev), torch.from_numpy(cond).to(dev), torch.from_numpy(eps).to(dev)
    eps_nchw = eps[:Fv].transpose(0, 3, 1, 2).astype(np.float32)
    for co in (R.ddim_coeffs(sch.alphas_cumprod, ts)[-1], R.ddim_coeffs(sch.alphas_cumprod, ts)[1]):
        c32 = [float(np.float32(c)) for c in co]
        for inversion in (True, False):
            x = torch.from_numpy(x0).to(dev)
            xin = torch.full((F + 2, h, w, 8), SENT, dtype=torch.float16, device=dev)     # two records beyond the group: never written
            L.tcl_invert_pack_f16(x, cond_d, idx, N, F, h, w, xin, stream())
            packed = xin.cpu().numpy()
            want = np.concatenate([x0[idx_h].astype(np.float16), cond[idx_h]], axis=1).transpose(0, 2, 3, 1)
            assert np.array_equal(packed[:F], want) and (packed[F:] == SENT).all()
            assert np.array_equal(x.cpu().numpy(), x0)                                   # the pack reads the master only
            L.tcl_ddim_step_f32(x, eps_d, idx, N, F, Fv, h, w, *c32, int(inversion), xin, stream())
            got, rec = x.cpu().numpy(), xin.cpu().numpy()
            new = R.ddim_step_ref(x0[idx_h[:Fv]], eps_nchw, co, inversion)
            assert np.array_equal(got[idx_h[:Fv]].view(np.uint32), new.view(np.uint32)), (h, w, inversion)
            absent = [n for n in range(N) if n not in idx_h[:Fv]]
            assert absent == [1, 4] and np.array_equal(got[absent], x0[absent])          # frames outside the group: untouched
            assert np.array_equal(rec[:Fv, ..., :4], new.astype(np.float16).transpose(0, 2, 3, 1))
            assert np.array_equal(rec[Fv:F], packed[Fv:F]) and (rec[F:] == SENT).all()   # the duplicate's record and the records beyond: untouched
            assert np.array_equal(rec[:F, ..., 4:], packed[:F, ..., 4:])                 # channels 4-7 are written once, by the pack
            if inversion:                                                                # ... followed by sampling with the same eps and coefficients
                L.tcl_ddim_step_f32(x, eps_d, idx, N, F, Fv, h, w, *c32, 0, xin, stream())
                back = x.cpu().numpy()[idx_h[:Fv]].astype(np.float64)
                tol = R.roundtrip_bound(x0[idx_h[:Fv]], eps_nchw, co)
                assert (np.abs(back - x0[idx_h[:Fv]]) <= tol).all()
    # TCL_EINVAL: F_valid = 0, F_valid > F, negative sizes, null pointers
    x = torch.from_numpy(x0).to(dev)
    xin = torch.zeros(F, h, w, 8, dtype=torch.float16, device=dev)
    ok = [x, eps_d, idx, N, F, Fv, h, w, *c32, 1, xin]
    for pos, bad in ((5, 0), (5, F + 1), (4, -1), (6, -h), (7, -w), (3, 0), (0, 0), (1, 0), (2, 0), (13, 0)):
        a = list(ok); a[pos] = bad
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_ddim_step_f32(*a, stream())
    okp = [x, cond_d, idx, N, F, h, w, xin]
    for pos, bad in ((4, 0), (4, -2), (5, -h), (6, 0), (3, -1), (0, 0), (1, 0), (2, 0), (7, 0)):
        a = list(okp); a[pos] = bad
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            L.tcl_invert_pack_f16(*a, stream())
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), x0)                                           # a refused call wrote nothing


# ---------------------------------------------------------------------------------------------------------------- 2. loop parity
def _report(line):
    print(line)
    out = os.environ.get("TCL_INVERT_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("h,w", [(16, 24), (10, 14)])
def test_inversion_and_recon_vs_oracle(setup, tmp_path, h, w):
    """Figures of an MI355X run: profiles/invert_parity.txt (engine, floor, ratio per plane and direction)."""
    sd, eng = setup
    g = np.random.default_rng(7 * h + w)
    lat = torch.from_numpy(g.standard_normal((N_FRAMES, 4, h, w)).astype(np.float32)).half()
    cond = torch.from_numpy(g.standard_normal((N_FRAMES, 4, h, w)).astype(np.float32)).half()
    cnd = torch.from_numpy(g.standard_normal((1, L_TEXT, 768)).astype(np.float32)).half()
    text = torch.cat([cnd, cnd])
    two = _inverter(eng, _config(tmp_path, h, w, max_tokens_per_pass=4 * h * w))          # 4 + 1 frames
    one = _inverter(eng, _config(tmp_path, h, w))                                         # 5 frames in 6 slots
    two.h, two.w = one.h, one.w = h, w
    assert [(f, v) for _, f, v in two._groups(N_FRAMES)] == [(4, 4), (2, 1)] and [(f, v) for _, f, v in one._groups(N_FRAMES)] == [(6, 5)]
    ts = two.timesteps()
    assert len(ts) == STEPS and ts[-1] == 999
    tome = eng.tome
    xe = two.ddim_inversion(lat, cond.cuda(), text.cuda())
    assert xe.dtype == torch.float32 and eng.tome is tome and tome.enabled                # f32 master; the generator's VidToMe is back, untouched
    ref = R.invert_ref(sd, lat, cond, text, ts)
    ref16 = R.invert_ref(sd, lat, cond, text, ts, half=True)
    r, floor = rel(xe, ref), rel(ref16, ref)
    _report(f"inversion {h}x{w} {N_FRAMES} frames {STEPS} steps: engine {r:.3e} floor {floor:.3e} ratio {r / floor:.3f}")
    # the way back, both from the f32 reference's inverted latents
    se = two.ddim_sample(ref.cuda(), cond.cuda(), text.cuda())
    sref = R.sample_ref(sd, ref, cond, text, ts)
    sref16 = R.sample_ref(sd, ref, cond, text, ts, half=True)
    rs, floors = rel(se, sref), rel(sref16, sref)
    _report(f"recon     {h}x{w} {N_FRAMES} frames {STEPS} steps: engine {rs:.3e} floor {floors:.3e} ratio {rs / floors:.3f}")
    assert r < MARGIN * floor, (r, floor)
    assert rs < MARGIN * floors, (rs, floors)
    # Group invariance: one group against two gives the same bits -- a wrong slot-to-frame mapping shows here.  Rows are independent, but at these row
    # counts the GEMMs' K-split count follows the group's size (gemm.hip split_rule; tests/test_gpu_unet.py::test_forward_many_equals_sequential), which
    # associates the f32 sums differently: the comparison runs with the split-K workspace taken away (one split everywhere), as test_gpu_kernels.py does.
    from tc_light_amd.lib import lib
    from tc_light_amd.unet import Ops
    ws = Ops._splitk_ws[str(eng.dev)]
    lib().tcl_set_workspace(0, 0)
    try:
        a, b = (i.ddim_inversion(lat, cond.cuda(), text.cuda()) for i in (one, two))
        assert torch.equal(a, b) and rel(a, xe.cpu()) < 1e-2
        a, b = (i.ddim_sample(ref.cuda(), cond.cuda(), text.cuda()) for i in (one, two))
        assert torch.equal(a, b)
        torch.cuda.synchronize()
    finally:
        lib().tcl_set_workspace(ws, ws.numel())


# ---------------------------------------------------------------------------------------------------------------- 3. producer meets consumer
def test_inverter_writes_what_the_generator_reads(setup, tmp_path, capsys):
    from PIL import Image
    from tc_light_amd import dataparser as D
    from tc_light_amd import sd15
    from tc_light_amd.generate import Generator
    from tc_light_amd.vae import VAEEngine
    _, eng = setup
    vae = VAEEngine(sd15.random_state_dict(sd15.vae_param_shapes(), seed=2), "cuda")
    n, H, W = 8, 64, 96
    frames_dir = tmp_path / "clip"
    frames_dir.mkdir()
    g = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        img = np.stack([127 + 100 * np.sin((xx + 7 * i) / 9.0 + c) * np.cos(yy / (5.0 + c)) for c in range(3)], -1) + g.integers(-8, 8, (H, W, 3))
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(frames_dir / f"{i:04d}.png")
    cfg = _config(tmp_path, H // 8, W // 8, rgb_path=str(frames_dir), recon=True)
    calls = []
    real = eng.forward_many
    eng.forward_many = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        inv = _inverter(eng, cfg, vae)
        x = inv(cfg.inversion.save_path)
        n_first = len(calls)
        assert inv(cfg.inversion.save_path) is None and len(calls) == n_first              # latents exist: the UNet is not run again
    finally:
        del eng.forward_many
    assert n_first == 2 * STEPS                                                            # one group; inversion + reconstruction
    assert "Skip inversion" in capsys.readouterr().out
    d = D.get_latents_dir(cfg.inversion.save_path, "iclight")
    saved = torch.load(os.path.join(d, "noisy_latents_999.pt"), weights_only=True)
    assert saved.dtype == torch.float16 and tuple(saved.shape) == (n, 4, H // 8, W // 8) and torch.equal(saved, x.half().cpu())
    assert torch.isfinite(saved.float()).all() and saved.float().std() > 0
    assert sorted(os.listdir(os.path.join(d, "recon_frames"))) == [f"{i:04d}.png" for i in range(n)]
    assert os.path.exists(os.path.join(d, "config.yaml")) and os.path.exists(os.path.join(d, "inversion_prompts.txt"))
    assert cfg.total_time > 0 and cfg.max_memory_allocated > 0
    ids = [1, 3, 4, 6]
    gen = Generator(eng, vae, dict(latents_path=cfg.inversion.save_path, model_key="iclight", frame_ids=ids, n_timesteps=STEPS, seed=41,
                                   max_tokens_per_pass=1 << 20))
    frames = inv.data_parser.load_video(ids)
    gen.prepare_data(frames)
    assert "latent path found" in capsys.readouterr().out
    assert gen.init_noise.dtype == torch.float16 and gen.init_noise.is_cuda and torch.equal(gen.init_noise.cpu(), saved[ids])
    fresh = torch.Generator(device=eng.dev).manual_seed(41)                                # nothing was drawn from the generator's RNG
    assert torch.equal(torch.randn(16, generator=gen.rng_dev, device=eng.dev), torch.randn(16, generator=fresh, device=eng.dev))
