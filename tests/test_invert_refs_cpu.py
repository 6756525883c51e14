"""CPU: DDIM inversion -- the references of tests/invert_refs.py pinned to the float64 transliteration of `pred_next_x`, the schedule facts the inverter
relies on, the host surface of `Inverter` on a stub engine (file names, skip unless force, save_intermediate, the timestep-mismatch error, the refusals,
the legacy `Inverter(None, None, cfg)` entry) and the two new symbols of the C ABI.
"""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import invert_refs as R
from tc_light_amd.config_utils import _plain, _wrap
from tc_light_amd.scheduler import DPMSolverSDEScheduler


# ---------------------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("inversion", [True, False])
def test_step_ref_matches_the_float64_transliteration(inversion):
    """Bound: invert_refs.step_bound -- 8 u m_b (|x| + |s_a eps|) / m_a + 3 u |s_b eps| with u = 2^-24, from the f32 roundings of the four scalars
    and of the product, difference, quotient, product, product, sum (derivation in its docstring): a few f32 ulps of the result's magnitude."""
    g = np.random.default_rng(3)
    sch = DPMSolverSDEScheduler()
    for n in (4, 25):
        sch.set_timesteps(n)
        ts = sorted(set(sch.timesteps.tolist()))
        for co in R.ddim_coeffs(sch.alphas_cumprod, ts):
            x = (g.standard_normal(4096) * 3).astype(np.float32)
            eps = g.standard_normal(4096).astype(np.float16).astype(np.float32)
            got, want = R.ddim_step_ref(x, eps, co, inversion), R.ddim_step_f64(x, eps, co, inversion)
            assert got.dtype == np.float32
            err, tol = np.abs(got.astype(np.float64) - want), R.step_bound(x, eps, co, inversion)
            assert (err <= tol).all(), (co, float((err / tol).max()))


def test_roundtrip_bound_holds_for_the_reference():
    g = np.random.default_rng(4)
    sch = DPMSolverSDEScheduler()
    sch.set_timesteps(4)
    ts = sorted(set(sch.timesteps.tolist()))
    for co in R.ddim_coeffs(sch.alphas_cumprod, ts):
        x = (g.standard_normal(4096) * 2).astype(np.float32)
        eps = g.standard_normal(4096).astype(np.float16).astype(np.float32)
        back = R.ddim_step_ref(R.ddim_step_ref(x, eps, co, True), eps, co, False)
        assert (np.abs(back.astype(np.float64) - x) <= R.roundtrip_bound(x, eps, co)).all()


# ---------------------------------------------------------------------------------------------------------------- the schedule
def test_schedule_facts():
    from tc_light_amd.invert import ddim_coeffs, inversion_timesteps
    sch = DPMSolverSDEScheduler()
    firsts = {}
    for n in (4, 20, 25):
        ts = inversion_timesteps(sch, n)
        assert all(b > a for a, b in zip(ts, ts[1:])), ts                      # reversed and de-duplicated: strictly increasing
        sch.set_timesteps(n)
        assert ts[-1] == int(sch.timesteps[0])
        assert sorted(set(sch.timesteps.tolist())) == ts                       # nothing but consecutive duplicates was dropped
        firsts[n] = ts[-1]
        for a, b in zip(ddim_coeffs(sch.alphas_cumprod, ts), R.ddim_coeffs(sch.alphas_cumprod, ts)):
            assert a == pytest.approx(b, rel=1e-15)
    assert len(set(firsts.values())) == 1 and firsts[25] == 999               # every pair of step counts names the same file
    assert np.array_equal(R.sd15_alphas_cumprod(), sch.alphas_cumprod)
    # a duplicated timestep is the identity: its level has (mu, sigma) == (mu_prev, sigma_prev), i.e. x -> 1 * x + 0 * eps
    mu, sigma, mu_p, sigma_p = R.ddim_coeffs(sch.alphas_cumprod, [10, 10])[1]
    assert (mu, sigma) == (mu_p, sigma_p)
    assert mu / mu_p == 1.0 and sigma - sigma_p * (mu / mu_p) == 0.0          # x_new = (mu/mu_p) x + (sigma - sigma_p mu/mu_p) eps
    # final_alpha_cumprod = alphas_cumprod[0]
    assert R.ddim_coeffs(sch.alphas_cumprod, [7])[0][2] == float(np.sqrt(sch.alphas_cumprod[0]))


# ---------------------------------------------------------------------------------------------------------------- host surface on a stub engine
H, W, NF = 16, 24, 5


def _config(tmp_path, **inv):
    frames = tmp_path / "frames"
    if not frames.exists():
        frames.mkdir()
        np.save(frames / "clip.npy", (np.random.default_rng(1).random((NF, H, W, 3)) * 255).astype(np.uint8))
    inversion = dict(save_path=str(tmp_path / "latents"), prompt="a street at dusk", n_frames=None, steps=4, save_intermediate=False, save_steps=4,
                     use_blip=False, recon=False, control="none", control_scale=1.0, batch_size=8, force=False, max_tokens_per_pass=1 << 20)
    inversion.update(inv)
    return _wrap(dict(sd_version="iclight", model_key="iclight", seed=3, work_dir=str(tmp_path), data=dict(scene_type="video", rgb_path=str(frames), height=H, width=W),
                      inversion=inversion, generation=dict(n_timesteps=4, use_lora=False, prompt=None), models=dict(allow_random=True)))


class _StubInverter:
    """Mixed into Inverter below: the three device operations in torch on the CPU."""
    def _pack(self, x, cond, idx, F):
        i = idx.long()
        return torch.cat([x[i].half(), cond[i]], dim=1).permute(0, 2, 3, 1).contiguous()

    def _step(self, x, eps, idx, F, F_valid, co, inversion, xin):
        i = idx.long()[:F_valid]
        new = R.ddim_step_ref(x[i].numpy(), eps[:F_valid].permute(0, 3, 1, 2).float().numpy(), co, inversion)
        x[i] = torch.from_numpy(new)
        xin[:F_valid, ..., :4] = x[i].half().permute(0, 2, 3, 1)


def _stub_inverter(cfg, scheduler=None):
    from tc_light_amd.invert import Inverter
    dev = torch.device("cpu")
    calls = []

    def forward_many(xin, Fs, Hh, Ww, t, text, cfg_pair=False):
        calls.append((tuple(xin.shape), list(Fs), t))
        assert text.shape[0] == 2 and torch.equal(text[0], text[1]) and not cfg_pair
        assert type(unet.tome).__name__ == "VidToMe" and unet.tome.enabled is False and unet.tome is not generator_tome
        return (xin[..., :4].float() * 0.25 + xin[..., 4:].float() * 0.5).half()

    generator_tome = SimpleNamespace(enabled=True, args={})
    unet = SimpleNamespace(dev=dev, tome=generator_tome, forward_many=forward_many)
    vae = SimpleNamespace(encode_imgs_batch=lambda fr, bs=2: torch.nn.functional.avg_pool2d(fr, 8)[:, [0, 1, 2, 0]].half(),
                          decode_latents_batch=lambda z, bs=2: torch.nn.functional.interpolate(z[:, :3].float(), scale_factor=8).clamp(0, 1))
    cls = type("StubInverter", (_StubInverter, Inverter), {})
    inv = cls(SimpleNamespace(unet=unet, vae=vae), scheduler or DPMSolverSDEScheduler(), cfg)
    return inv, calls, unet, generator_tome


def test_files_skip_force_and_intermediates(tmp_path, capsys):
    from tc_light_amd import dataparser as D
    cfg = _config(tmp_path)
    inv, calls, unet, gtome = _stub_inverter(cfg)
    x = inv(cfg.inversion.save_path)
    d = D.get_latents_dir(cfg.inversion.save_path, "iclight")
    ts = inv.timesteps()
    assert unet.tome is gtome and gtome.enabled is True                        # the generator's instance: put back, never flipped
    assert sorted(os.listdir(d)) == ["config.yaml", "inversion_prompts.txt", f"noisy_latents_{ts[-1]}.pt"] and ts[-1] == 999
    saved = D.load_latent(d, ts[-1])
    assert saved.dtype == torch.float16 and saved.device.type == "cpu" and tuple(saved.shape) == (NF, 4, H // 8, W // 8)
    assert x.dtype == torch.float32 and torch.equal(saved, x.half())           # the master is f32; the file is its f16 image
    assert open(os.path.join(d, "inversion_prompts.txt")).read().split("\n") == ["a street at dusk"] * NF
    import yaml
    written = yaml.safe_load(open(os.path.join(d, "config.yaml")))
    assert "generation" not in written and written["inversion"]["steps"] == 4
    assert cfg.total_time > 0
    # one group of 5 frames: 6 physical slots (the odd duplicate), one pass per level, eps at the level being stepped to
    assert [c[0] for c in calls] == [(6, H // 8, W // 8, 8)] * len(ts) and [c[1] for c in calls] == [[3]] * len(ts) and [c[2] for c in calls] == ts
    # the loop against the reference restated here (same stub UNet)
    lat = torch.nn.functional.avg_pool2d(inv.data_parser.load_video(), 8)[:, [0, 1, 2, 0]].half()
    want = lat.float().numpy()
    for co in R.ddim_coeffs(inv.scheduler.alphas_cumprod, ts):
        eps = (torch.from_numpy(want).half().float() * 0.25 + lat.float() * 0.5).half().float().numpy()
        want = R.ddim_step_ref(want, eps, co, True)
    assert np.array_equal(x.numpy(), want)
    # a second call without force: the UNet is not run
    n = len(calls)
    assert inv(cfg.inversion.save_path) is None and len(calls) == n
    assert "Skip inversion" in capsys.readouterr().out
    cfg.inversion.force = True
    inv2, calls2, _, _ = _stub_inverter(cfg)
    inv2(cfg.inversion.save_path)
    assert len(calls2) == len(ts)
    # two groups (4 + 1 frames: the second one is a lone frame and its duplicate) give the same bits; batch_size is only an upper bound
    for kw in (dict(max_tokens_per_pass=4 * (H // 8) * (W // 8)), dict(batch_size=4)):
        cfg3 = _config(tmp_path, force=True, **kw)
        inv3, calls3, _, _ = _stub_inverter(cfg3)
        assert torch.equal(inv3(cfg3.inversion.save_path), x)
        assert [c[0][0] for c in calls3] == [4, 2] * len(ts)
    # n_frames cuts the video; save_intermediate writes every save_steps timestep that is visited
    os.makedirs(tmp_path / "b", exist_ok=True)
    cfg4 = _config(tmp_path / "b", n_frames=3, save_intermediate=True, recon=True)
    inv4, _, _, _ = _stub_inverter(cfg4)
    inv4(cfg4.inversion.save_path)
    d4 = D.get_latents_dir(cfg4.inversion.save_path, "iclight")
    assert {f for f in os.listdir(d4) if f.endswith(".pt")} == {f"noisy_latents_{t}.pt" for t in ts}
    assert tuple(D.load_latent(d4, ts[0]).shape) == (3, 4, H // 8, W // 8)
    assert sorted(os.listdir(os.path.join(d4, "recon_frames"))) == ["0000.png", "0001.png", "0002.png"]
    assert "PSNR" in capsys.readouterr().out
    assert inv4.check_latent_exists(d4) and not inv2.check_latent_exists(d4 + "_absent")


def test_mismatched_first_timesteps_raise(tmp_path):
    class Doctored(DPMSolverSDEScheduler):
        def set_timesteps(self, n, device=None):
            super().set_timesteps(n)
            if n == 7:
                self.timesteps = self.timesteps.clone()
                self.timesteps[0] = 981

    cfg = _config(tmp_path)
    cfg.generation.n_timesteps = 7
    inv, calls, _, _ = _stub_inverter(cfg, Doctored())
    with pytest.raises(ValueError, match=r"999.*981|981.*999"):
        inv(cfg.inversion.save_path)
    assert not calls and not os.path.exists(os.path.join(cfg.inversion.save_path, "iclight", "noisy_latents_999.pt"))


@pytest.mark.parametrize("change", ["control", "use_blip", "sd_version", "world", "carla"])
def test_refusals_come_before_any_model_is_loaded(tmp_path, monkeypatch, change):
    import yaml
    import invert as top
    cfg = _config(tmp_path)
    if change == "control":
        cfg.inversion.control = "depth"
    elif change == "use_blip":
        cfg.inversion.use_blip = True
    elif change == "sd_version":
        cfg.sd_version = "2.1"
    elif change == "carla":
        cfg.data.scene_type = "carla"
    else:
        monkeypatch.setenv("WORLD_SIZE", "2")
    path = tmp_path / "cfg.yaml"
    yaml.safe_dump(_plain(cfg), open(path, "w"))

    def no_model(*a, **k):
        raise AssertionError("a model was loaded before the refusal")
    monkeypatch.setattr(top, "init_iclight", no_model)
    with pytest.raises(NotImplementedError):
        top.main(["--config", str(path)])
    with pytest.raises(NotImplementedError):                                   # ... and the class refuses too, whoever builds it
        _stub_inverter(cfg)


def test_legacy_entry_keeps_printing_and_returning(tmp_path, capsys):
    from invert import Inverter
    from tc_light_amd.invert import Inverter as Engine
    assert Inverter is Engine
    cfg = _config(tmp_path)
    assert Inverter(None, None, cfg)(cfg.inversion.save_path) is None
    assert capsys.readouterr().out.strip() == "[INFO] sd_version 'iclight': no inversion needed, latents start from noise (reference run.py:13-22)"
    assert not os.path.exists(cfg.inversion.save_path)
    cfg.sd_version = "1.5"
    with pytest.raises(NotImplementedError):
        Inverter(None, None, cfg)(cfg.inversion.save_path)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH, parse_header
    if not os.path.exists(LIB_PATH):
        g.build()
    sig = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("tcl_invert_pack_f16", 9), ("tcl_ddim_step_f32", 15)):
        assert name in sig and len(sig[name][1]) == nargs and hasattr(dll, name), name
