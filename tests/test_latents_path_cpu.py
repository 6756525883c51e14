"""CPU: `generation.latents_path` -- the restatement of the reference's `get_latents_dir` / `check_latent_exists` / `load_latent`
(tc_light_amd/dataparser.py) against tests/golden/latents.npz, which the reference's own functions wrote (tests/golden/make_golden_latents.py),
and `Generator.prepare_data`'s use of it: an absent file changes nothing (the start noise and the RNG stream are the parent's), a present one
becomes `init_noise` (f16, this run's frames), a wrong shape raises.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tc_light_amd import dataparser as D


@pytest.fixture(scope="module")
def g(golden):
    return golden("latents")


def test_directory_file_name_and_frame_selection_match_the_reference(g, tmp_path):
    root = str(tmp_path)
    for key, name in zip(g["model_keys"].tolist(), g["dir_names"].tolist()):
        assert os.path.relpath(D.get_latents_dir(root, key or None), root) == name
    ts = torch.from_numpy(g["timesteps"])
    d = D.get_latents_dir(root, "iclight")
    os.makedirs(d)
    assert os.path.basename(D.latent_file(d, ts[0])) == str(g["file_name_tensor_t"])          # timesteps[0] is a 0-dim tensor
    assert os.path.basename(D.latent_file(d, int(ts[1]))) == str(g["file_name_int_t"])
    assert D.check_latent_exists(d, [ts[0]]) == bool(g["exists_before"]) is False
    with pytest.raises(FileNotFoundError):
        D.load_latent(d, ts[0])
    torch.save(torch.from_numpy(g["latents"]), os.path.join(d, str(g["file_name_tensor_t"])))
    assert D.check_latent_exists(d, [ts[0]]) == bool(g["exists_after"]) is True
    assert not D.check_latent_exists(d, [ts[0], ts[1]])                                         # every asked timestep needs its file
    ids = g["frame_ids"].tolist()
    sel = D.load_latent(d, ts[0], ids)
    assert sel.dtype == torch.float32 and np.array_equal(sel.numpy(), g["selected"])
    assert np.array_equal(D.load_latent(d, ts[0]).numpy(), g["selected_all"])
    assert np.array_equal(g["selected"], g["latents"][ids])


def _generator(cfg, rank=0, world=1):
    from tc_light_amd.generate import Generator
    from tc_light_amd.parallel import Dist
    dev = torch.device("cpu")
    stub = SimpleNamespace(dev=dev, tome=SimpleNamespace(args={}))
    return Generator(stub, None, dict(cfg, max_tokens_per_pass=1 << 20), dist=Dist(rank, world))


def _parent_noise(mode, n, h, w, seed):
    """prepare_data's start noise as the parent commit draws it (generate.py:183-188), restated."""
    rng = torch.Generator(device="cpu").manual_seed(seed)
    if mode == "same":
        z = torch.randn(1, 4, h, w, generator=rng, dtype=torch.float32).to(torch.float16).repeat(n, 1, 1, 1)
    else:
        z = torch.randn(n, 4, h, w, generator=rng, dtype=torch.float32).to(torch.float16)
    return z, torch.randn(n, 4, h, w, generator=rng, dtype=torch.float32)                       # ... and the next draw of the same stream


@pytest.mark.parametrize("mode", ["same", "vanilla"])
def test_absent_file_leaves_noise_and_rng_stream_as_they_were(tmp_path, capsys, mode):
    n, h, w = 3, 2, 3
    frames = torch.zeros(n, 3, 8 * h, 8 * w)
    want, want_next = _parent_noise(mode, n, h, w, 41)
    for lp in (None, str(tmp_path / "latents")):                                                # no key at all; a key whose directory holds nothing
        gen = _generator(dict(noise_mode=mode, seed=41, n_timesteps=3, latents_path=lp, model_key="iclight", frame_ids=[0, 1, 2]))
        gen.prepare_data(frames)
        assert gen.init_noise.dtype == torch.float16 and torch.equal(gen.init_noise, want)
        assert torch.equal(torch.randn(n, 4, h, w, generator=gen.rng_dev, dtype=torch.float32), want_next)
        out = capsys.readouterr().out
        assert ("latent path not found, generating new latents." in out) == (lp is not None)


def test_present_file_becomes_init_noise_and_wrong_shape_raises(tmp_path, capsys):
    from tc_light_amd.scheduler import DPMSolverSDEScheduler
    h, w, ids = 2, 3, [1, 2, 4, 5]
    sch = DPMSolverSDEScheduler()
    sch.set_timesteps(3)
    d = D.get_latents_dir(str(tmp_path), "iclight")
    os.makedirs(d)
    saved = torch.randn(7, 4, h, w, generator=torch.Generator().manual_seed(2)) * 3
    torch.save(saved, D.latent_file(d, sch.timesteps[0]))
    cfg = dict(noise_mode="same", seed=41, n_timesteps=3, latents_path=str(tmp_path), model_key="iclight", frame_ids=ids)
    gen = _generator(cfg)
    gen.prepare_data(torch.zeros(4, 3, 8 * h, 8 * w))
    assert f"latent path found at {d}" in capsys.readouterr().out
    assert gen.init_noise.dtype == torch.float16 and gen.init_noise.is_contiguous()
    assert torch.equal(gen.init_noise, saved[ids].to(torch.float16))
    # two ranks: each takes its block of the selected frames
    for rank in (0, 1):
        gr = _generator(cfg, rank, 2)
        gr.n_total = 4
        gr.prepare_data(torch.zeros(2, 3, 8 * h, 8 * w))
        lo, hi = gr.dist.range(4)
        assert torch.equal(gr.init_noise, saved[ids][lo:hi].to(torch.float16))
    # frame_ids None: the whole file is this run's
    gen = _generator(dict(cfg, frame_ids=None))
    gen.prepare_data(torch.zeros(7, 3, 8 * h, 8 * w))
    assert torch.equal(gen.init_noise, saved.to(torch.float16))
    # refusals: another latent size, another frame count, another channel count, ids past the file
    for frames, c in ((torch.zeros(4, 3, 8 * h, 8 * (w + 1)), cfg), (torch.zeros(3, 3, 8 * h, 8 * w), cfg),
                      (torch.zeros(4, 3, 8 * h, 8 * w), dict(cfg, frame_ids=[0, 1, 2, 9]))):
        with pytest.raises(ValueError):
            _generator(c).prepare_data(frames)
    torch.save(saved[:, :3], D.latent_file(d, sch.timesteps[0]))
    with pytest.raises(ValueError):
        _generator(cfg).prepare_data(torch.zeros(4, 3, 8 * h, 8 * w))
