"""CPU: the numpy reference of generation.noise_mode warp (tests/noisewarp_refs.py) pinned from both sides -- its f32 sequence against float64, the
identities the definition promises bit for bit, and the statistics of the latent noise against bounds derived for n samples of white unit-variance
noise: 5 / sqrt(n) on the mean and the neighbour covariances, 5 sqrt(2 / n) on the variance (noisewarp_refs.bounds).  The naive transport must fall
outside them.  Then hostlogic.check_noise_warp.

Measured here (256x256, n = 4096, after four steps; mean, variance, horizontal / vertical covariance): see the line each statistics test prints."""
import numpy as np
import pytest

import noisewarp_refs as R


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def zooms():
    """name -> (z of the chain, z of the naive chain), 256x256, five frames = four steps."""
    N, H, W = 5, 256, 256
    G = R.fields(N, H, W, seed=1)
    out = {}
    for name, s in (("2x", 2.0), ("1.1x", 1.1)):
        f, m = R.zoom(N, H, W, s), R.ones(N, H, W)
        out[name] = (R.chain(G, f, m), R.chain(G, f, m, naive=True))
    return out


@pytest.mark.parametrize("name", ["zero", "integer", "half", "zoom_in", "zoom_out", "one_source", "nonfinite", "mask_edge"])
def test_f32_sequence_against_float64(name):
    """Every latent sample of the f32 sequence lies within the derived bound of the float64 chain (the same source map: q is defined in f32); the
    largest distance in units of the f32 spacing at 1 is printed."""
    N, H, W = 4, 72, 136
    G = R.fields(N, H, W, seed=2)
    f, m = R.cases(N, H, W)[name]
    z32 = R.chain(G, f, m)
    z64, bound = R.chain(G, f, m, f64=True, detail=True)
    assert z32.dtype == np.float32 and z64.dtype == np.float64
    err = np.abs(z32.astype(np.float64) - z64)
    print(f"{name}: max |z32 - z64| = {err.max():.3e} = {err.max() / 2.0 ** -23:.2f} ulp(1), max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_zero_flow_keeps_every_frame():
    N, H, W = 4, 64, 64
    z = R.chain(R.fields(N, H, W), R.translation(N, H, W, 0, 0), R.ones(N, H, W))
    for t in range(1, N):
        assert np.array_equal(bits(z[t]), bits(z[0]))


def test_eight_pixel_translation_shifts_one_latent_column():
    N, H, W = 4, 64, 72
    G = R.fields(N, H, W)
    z = R.chain(G, R.translation(N, H, W, 8, 0), R.ones(N, H, W))          # flow (-8, 0)
    for t in range(1, N):
        assert np.array_equal(bits(z[t][:, :, 1:]), bits(z[t - 1][:, :, :-1]))
        assert np.array_equal(bits(z[t][:, :, 0]), bits(R.reduce8(G[t])[:, :, 0]))      # the column that enters is fresh


def test_mask_zero_is_the_per_frame_reduction():
    N, H, W = 3, 64, 64
    G = R.fields(N, H, W)
    z = R.chain(G, R.zoom(N, H, W, 1.3), np.zeros((N, 1, H, W), dtype=np.float32))
    assert np.array_equal(bits(z), bits(np.stack([R.reduce8(g) for g in G])))


def test_ties_round_to_even_and_nonfinite_flows_are_invalid():
    f = np.zeros((2, 8, 8), dtype=np.float32)
    f[0] = 0.5                                                   # x + 0.5: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ...
    q = R.source_map(f, np.ones((8, 8), dtype=np.float32))
    assert q[0].tolist() == [0, 2, 2, 4, 4, 6, 6, -1]           # 7.5 -> 8 is outside
    f[0, 0, :4] = [np.nan, np.inf, -np.inf, 3e38]
    assert R.source_map(f, np.ones((8, 8), dtype=np.float32))[0, :4].tolist() == [-1, -1, -1, -1]
    m = np.full((8, 8), 0.5, dtype=np.float32)
    assert (R.source_map(np.zeros_like(f), m) == -1).all()       # exactly 0.5 is not > 0.5
    m[:] = np.nextafter(np.float32(0.5), np.float32(1))
    assert (R.source_map(np.zeros_like(f), m) >= 0).all()


def test_stretched_source_is_shared_exactly():
    """k pixels of one source: their normalised sum gives the source back (the conditional sample), up to rounding."""
    N, H, W = 2, 8, 8
    G = R.fields(N, H, W, seed=5)
    z, Fs, ks, Ss = R.chain(G, R.one_source(N, H, W), R.ones(N, H, W), detail=True)
    assert ks[1].max() == H * W and ks[1].sum() == H * W
    src = Fs[0][:, H // 2, W // 3].astype(np.float64)
    back = Fs[1].astype(np.float64).sum(axis=(1, 2)) / np.sqrt(H * W)
    assert np.abs(back - src).max() < 1e-5


@pytest.mark.parametrize("name", ["2x", "1.1x"])
def test_zoom_statistics(zooms, name):
    z, naive = zooms[name]
    bm, bv = R.bounds(z[0].size)
    for t in range(z.shape[0]):
        m, v, ch, cv = R.stats(z[t])
        print(f"zoom {name} frame {t}: mean {m:+.4f} var {v:.4f} cov h {ch:+.4f} v {cv:+.4f}  (bounds {bm:.4f} / {bv:.4f})")
        assert abs(m) <= bm and abs(v - 1.0) <= bv and abs(ch) <= bm and abs(cv) <= bm
    m, v, ch, cv = R.stats(naive[-1])
    print(f"zoom {name} naive, last frame: mean {m:+.4f} var {v:.4f} cov h {ch:+.4f} v {cv:+.4f}")
    assert abs(v - 1.0) > bv and not R.white(naive[-1])        # the copies pile up: the variance leaves the bound at either zoom


def test_three_pixel_translation_correlates_by_the_block_overlap():
    N, H, W = 2, 256, 256
    z = R.chain(R.fields(N, H, W, seed=6), R.translation(N, H, W, 3, 0), R.ones(N, H, W)).astype(np.float64)
    a, b = z[1] - z[1].mean(), z[0] - z[0].mean()
    corr = float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))
    print(f"correlation of z_1 with z_0 under a 3 px translation: {corr:.4f} (5/8 = 0.625)")
    assert abs(corr - 5.0 / 8.0) <= R.bounds(z[0].size)[0]


# ---------------------------------------------------------------------------------------------------------------- hostlogic
def test_check_noise_warp():
    from tc_light_amd import hostlogic as HL
    assert HL.check_noise_warp("warp") == dict(steps=True)
    assert HL.check_noise_warp("WARP", dict(steps=False)) == dict(steps=False)
    for mode in ("same", "vanilla", "mixed", None):              # the block is not even looked at
        assert HL.check_noise_warp(mode, dict(nonsense=1), keyframes=dict(interval=2), highres_scale=2.0, normal=True) is None
    for block, word in ((dict(step=True), "generation.noise_warp"), ([True], "generation.noise_warp"), (dict(steps=1), "generation.noise_warp.steps"),
                        (dict(steps="yes"), "generation.noise_warp.steps")):
        with pytest.raises(ValueError, match=word):
            HL.check_noise_warp("warp", block)
    for kw, word in ((dict(keyframes=dict(interval=2)), "generation.keyframes"), (dict(highres_scale=1.5), "generation.highres_scale"),
                     (dict(normal=True), "generation.normal")):
        with pytest.raises(ValueError) as e:
            HL.check_noise_warp("warp", None, **kw)
        assert "generation.noise_mode" in str(e.value) and word in str(e.value)


def test_resolve_generation_with_and_without_warp():
    from tc_light_amd import hostlogic as HL
    from tc_light_amd.generate import DEFAULTS
    base = HL.resolve_generation(dict(DEFAULTS))
    assert "noise_warp" not in base
    for mode in ("same", "vanilla"):                             # as before, whatever the block says
        assert HL.resolve_generation(dict(DEFAULTS, noise_mode=mode, noise_warp=dict(steps=False))) == base
    assert HL.resolve_generation(dict(DEFAULTS, noise_mode="warp")) == dict(base, noise_warp=dict(steps=True))
    assert HL.resolve_generation(dict(DEFAULTS, noise_mode="warp", noise_warp=dict(steps=False)))["noise_warp"] == dict(steps=False)
    for over, word in ((dict(keyframes=4), "generation.keyframes"), (dict(highres_scale=2.0), "generation.highres_scale"),
                       (dict(normal=True, iclight_model="fbc", apply_opt=False), "generation.normal")):
        with pytest.raises(ValueError) as e:
            HL.resolve_generation(dict(DEFAULTS, noise_mode="warp", **over))
        assert "generation.noise_mode" in str(e.value) and word in str(e.value)


def test_cli_flags(tmp_path):
    import os
    from tc_light_amd.config_utils import load_config
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    cfg = tmp_path / "c.yaml"
    cfg.write_text(f"base_config: {os.path.join(root, 'configs', 'tclight_default.yaml')}\nwork_dir: {tmp_path}\n")
    c = load_config(["--config", str(cfg)], print_config=False)
    assert c.generation.noise_mode == "same" and c.generation.get("noise_warp") is None
    c = load_config(["--config", str(cfg), "--noise_mode", "warp", "--noise_warp_steps", "0"], print_config=False)
    assert c.generation.noise_mode == "warp" and dict(c.generation.noise_warp) == dict(steps=False)
    ex = load_config(["--config", os.path.join(root, "configs", "examples", "tclight_noise_warp.yaml")], print_config=False)
    assert ex.generation.noise_mode == "warp" and dict(ex.generation.noise_warp) == dict(steps=True)
