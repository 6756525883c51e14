"""CPU: the product's host logic (tc_light_amd/hostlogic.py) against the goldens produced by the reference's own code."""
import numpy as np
import torch

from tc_light_amd import hostlogic as HL


def test_chunks_match_reference(golden):
    g = golden("pipeline")
    for tag, flen in {"n8": 8, "n30": 30, "n300": 300, "w120": 120, "n3": 3}.items():
        rf, fl = g[f"chunks_{tag}_draws"]
        ch = HL.chunks_from_draws(flen, 4, int(rf), float(fl), torch.from_numpy(g[f"chunks_{tag}_perm"]))
        assert [c for chunk in ch for c in chunk] == list(g[f"chunks_{tag}_flat"])
        assert [len(c) for c in ch] == list(g[f"chunks_{tag}_lens"])
        assert HL.n_chunks(flen, 4, int(rf)) == len(ch)


def test_chunk_sampler_covers_everything():
    s = HL.ChunkSampler(12345)
    for flen in (1, 2, 5, 30, 38, 120, 160):
        for _ in range(5):
            ch = s.get_chunks(flen)
            flat = sorted(c for chunk in ch for c in chunk)
            assert flat == list(range(flen)) and all(1 <= len(c) <= 4 for c in ch)


def test_windows_alpha_shards(golden):
    g = golden("pipeline")
    assert HL.temporal_windows(300, 64) == ([0, 59, 118, 177, 236], [5, 5, 5, 5])
    assert HL.temporal_windows(30, 64) == ([0], [0]) and HL.temporal_windows(64, 64) == ([0], [0])
    for n in (8, 30, 64, 65, 127, 300):
        starts, _ = HL.temporal_windows(n, 64)
        assert starts == sorted({int(s) for s, _ in g[f"tden_{n}_windows"]})
    np.testing.assert_allclose(HL.alpha_schedule(0.01, 0.01, 20), g["ddim_alphas"], rtol=1e-12)
    sizes = [HL.shard_range(300, r, 8) for r in range(8)]
    assert [b - a for a, b in sizes] == [38, 38, 38, 38, 37, 37, 37, 37] and sizes[0][0] == 0 and sizes[-1][1] == 300


def test_shard_track_ids_equal_fresh_flowid():
    """Multi-GPU stage 2 runs on each rank's frame block with the GLOBAL track ids restricted to the block and renumbered densely
    (generate.py of this repo, `shard_post_opt`).  That is the partition get_flowid (flow_utils.py:56-93) gives when started at the
    block's first frame -- i.e. the reference run on the shard."""
    import torch
    import synth
    from oracle import path2 as O2
    n, h, w = 7, 40, 56
    d = synth.video_clip(n, h, w, seed=4)
    frames = d["frames"].clone()
    frames[:, :, 0, 0] = 1.0                                   # same max in every block -> same colour threshold
    fwd = torch.zeros(n, 2, h, w)
    fwd[:, 0], fwd[:, 1] = -1.5, -0.5                          # forward flow of the synthetic translation
    fwd += 0.05 * torch.randn(fwd.shape, generator=torch.Generator().manual_seed(1))
    masks = d["masks"]
    ids = O2.get_flowid(frames, fwd, masks)
    for lo, hi in ((0, 4), (4, 7), (2, 6)):
        _, local = torch.unique(ids[lo:hi].reshape(-1), return_inverse=True)
        fresh = O2.get_flowid(frames[lo:hi], fwd[lo:hi], masks[lo:hi]).reshape(-1)
        # same partition <=> the pairing (local id, fresh id) is one-to-one
        pairs = torch.unique(torch.stack([local, fresh], 1), dim=0)
        assert pairs.shape[0] == local.max().item() + 1 == fresh.max().item() + 1


def test_bench_gpus_n_without_gpu_fails_loudly():
    """`python bench.py --gpus 2` on a box without GPUs must say so (exit != 0, one clear line) -- never run a silent 1-rank or CPU pass."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("GPU present")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "needs a GPU" in (p.stderr + p.stdout)


def test_run_groups_one_pass_per_group():
    """`Generator._run_groups` makes one `forward_many` call per group, with the group's chunk lengths in order."""
    from types import SimpleNamespace
    from tc_light_amd.generate import Generator
    calls = []
    unet = SimpleNamespace(forward_many=lambda x, Fs, *r, **k: calls.append(("one", Fs)) or "e")
    gen = SimpleNamespace(unet=unet)
    chunks = [list(range(3)), list(range(3, 19)), list(range(19, 35)), list(range(35, 40))]      # 3 + 16 + 16 + 5 frames
    pack = lambda grp: (None, None, sum(len(c) for c in grp))
    Generator._run_groups(gen, [chunks], 8, 8, 1.0, None, pack, lambda *a: None)
    assert calls == [("one", [3, 16, 16, 5])]


UNET_SWITCHES = dict(gn_concat="TCL_GN_CONCAT", ln_metric="TCL_LN_METRIC", qkv_panel="TCL_QKV_PANEL", merge_lazy="TCL_MERGE_LAZY", ln_gemm="TCL_LN_GEMM",
                     qpanel="TCL_QPANEL", tome_stream="TCL_TOME_STREAM", cfg_dedup="TCL_CFG_DEDUP")


def test_unet_switches_from_env(monkeypatch):
    """Names, defaults and the `!= "0"` rule of the eight UNet switches: on by default, "0" turns exactly its own field off, "1" is the same as unset."""
    from tc_light_amd.unet import Switches
    assert Switches._fields == tuple(UNET_SWITCHES)
    for var in UNET_SWITCHES.values():
        monkeypatch.delenv(var, raising=False)
    default = Switches.from_env()
    assert default == Switches(*[True] * 8)
    for field, var in UNET_SWITCHES.items():
        monkeypatch.setenv(var, "0")
        assert Switches.from_env() == default._replace(**{field: False}), var
        monkeypatch.setenv(var, "1")
        assert Switches.from_env() == default, var
        monkeypatch.delenv(var)


def test_environment_is_read_in_the_stated_places_only():
    """The UNet pass reads its switches once, at its top: `os.environ` appears in unet.py only in Switches.from_env and load_gemm_table -- never in the
    code that runs per block or per chunk -- and vidtome.py reads no environment at all."""
    import inspect
    from tc_light_amd import unet, vidtome
    fns = (unet.Switches.from_env.__func__, unet.load_gemm_table)
    inside = [inspect.getsource(f).count("os.environ") for f in fns]
    assert all(n > 0 for n in inside) and inspect.getsource(unet).count("os.environ") == sum(inside), inside
    assert "os.environ" not in inspect.getsource(vidtome)
