"""CPU: the float64 reference and the derived bound of generation.detail_transfer (tests/detail_refs.py), pinned from both sides -- the reference
against torch's float64 conv2d on reflect-padded input and against the closed form S - G(S) + G(R); an f32 emulation of the kernel's arithmetic lands
inside the bound on every case of the table, four planted defects land outside it."""
import numpy as np
import pytest
import torch

import detail_refs as R

GEOMS = sorted(R.geometries())


def _conv_blur(x, taps):
    """G in float64 through torch: two depthwise conv2d on reflect-padded input."""
    w = torch.from_numpy(np.asarray(taps, dtype=np.float64))
    r = (len(w) - 1) // 2
    t = torch.from_numpy(x)
    C = t.shape[1]
    t = torch.nn.functional.conv2d(torch.nn.functional.pad(t, (r, r, 0, 0), mode="reflect"), w.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)
    t = torch.nn.functional.conv2d(torch.nn.functional.pad(t, (0, 0, r, r), mode="reflect"), w.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return t.numpy()


def test_taps_are_the_wrappers():
    from tc_light_amd import detail
    for sigma in (0.5, 1.0, 1.5, 3.0, 16.0):
        w, r = detail.gaussian_taps(sigma)
        w2, r2 = R.taps_f32(sigma)
        assert r == r2 == int(np.ceil(3 * sigma)) and np.array_equal(w.numpy(), w2) and w.dtype == torch.float32
        assert abs(float(w2.astype(np.float64).sum()) - 1.0) < (2 * r + 1) * R.U and (w2 >= 0).all() and np.array_equal(w2, w2[::-1])
    assert detail.MAX_RADIUS == 48 == detail.radius_of(16.0)
    for bad in (0.49, 16.5, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            detail.gaussian_taps(bad)


@pytest.mark.parametrize("name", GEOMS)
def test_blur_agrees_with_conv2d(name):
    S, _, _, sigma = R.inputs(name)
    taps, r = R.taps_f32(sigma)
    a, b = R.blur(S.astype(np.float64), taps), _conv_blur(S.astype(np.float64), taps)
    assert a.shape == S.shape and np.abs(a - b).max() < 1e-14
    assert np.array_equal(R.reflect_index(5, 2), [2, 1, 0, 1, 2, 3, 4, 3, 2])          # the edge sample is not repeated


@pytest.mark.parametrize("name", GEOMS)
def test_add_rgb_at_full_strength_is_the_closed_form(name):
    S, Rl, _, sigma = R.inputs(name)
    taps, _ = R.taps_f32(sigma)
    ref, _ = R.reference(S, Rl, None, sigma, "add", "rgb", 1.0)
    S64, R64 = S.astype(np.float64), Rl.astype(np.float64)
    want = np.clip(S64 - _conv_blur(S64, taps) + _conv_blur(R64, taps), 0.0, 1.0)
    assert np.abs(ref - want).max() < 1e-13


@pytest.mark.parametrize("mode,channels", R.SETTINGS)
@pytest.mark.parametrize("name", GEOMS)
def test_reference_against_conv2d_composition(name, mode, channels):
    """The whole reference, every setting, against the same maths composed from conv2d."""
    c = R.case(name, mode, channels)
    taps, _ = R.taps_f32(c["sigma"])
    S, Rl = c["S"].astype(np.float64), c["R"].astype(np.float64)
    m = 1.0 if c["mask"] is None else c["mask"].astype(np.float64)
    Y = lambda x: (0.299 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2])[:, None]
    if mode == "add":
        D = Y(S - Rl) if channels == "luma" else S - Rl
        X = D - _conv_blur(D, taps)
    else:
        a, b = (Y(Rl), Y(S)) if channels == "luma" else (Rl, S)
        X = S * (_conv_blur(a, taps) + 1 / 255) / (_conv_blur(b, taps) + 1 / 255) - Rl
    want = np.clip(Rl + R.BLEND * m * X, 0.0, 1.0)
    assert np.abs(c["ref"] - want).max() < 1e-12
    assert np.abs(c["ref"] - Rl).max() > 1e-2                    # the step does something on these inputs


@pytest.mark.parametrize("mode,channels", R.SETTINGS)
@pytest.mark.parametrize("name", GEOMS)
def test_f32_emulation_inside_the_bound(name, mode, channels):
    c = R.case(name, mode, channels)
    got = R.emulate_f32(c["S"], c["R"], c["mask"], c["sigma"], mode, channels, R.BLEND)
    err = np.abs(got.astype(np.float64) - c["ref"])
    print(f"{name} {mode} {channels}: max err {err.max():.3e}, max err/bound {(err / np.maximum(c['bound'], 1e-300)).max():.3f}, "
          f"max bound {c['bound'].max():.3e}")
    assert (err <= c["bound"]).all()
    # the bound stays near f32 rounding: about 2 gamma(97) = 1.2e-5 of the signal at the largest radius, times S / (G(S) + e) <= 255 for ratio
    assert c["bound"].max() < (1e-3 if mode == "ratio" else 1e-5)


def _defects(c):
    taps, r = R.taps_f32(c["sigma"])
    k = np.arange(-r, r + 1, dtype=np.float64)
    raw = np.exp(-(k * k) / (2.0 * c["sigma"] ** 2))
    short = raw[1:-1] / raw[1:-1].sum()
    return {"edge_repeating_borders": dict(index=R.repeat_index),
            "unnormalised_taps": dict(taps=raw.astype(np.float32)),
            "radius_off_by_one": dict(taps=short.astype(np.float32)),
            "mask_ignored": dict(use_mask=False)}


@pytest.mark.parametrize("defect", ["edge_repeating_borders", "unnormalised_taps", "radius_off_by_one", "mask_ignored"])
@pytest.mark.parametrize("mode,channels", R.SETTINGS)
def test_planted_defects_land_outside_the_bound(mode, channels, defect):
    """On the case table's own inputs: every geometry the defect applies to (mask_ignored: the masked ones) shows it."""
    seen = 0
    for name in GEOMS:
        c = R.case(name, mode, channels)
        if defect == "mask_ignored" and c["mask"] is None:
            continue
        got = R.emulate_f32(c["S"], c["R"], c["mask"], c["sigma"], mode, channels, R.BLEND, **_defects(c)[defect])
        err = np.abs(got.astype(np.float64) - c["ref"])
        assert (err > c["bound"]).any(), f"{defect} stays inside the bound on {name}"
        assert (err > 10.0 * c["bound"]).any(), f"{defect} on {name}: nowhere beyond 10 x the bound"      # and not by a hair
        seen += 1
    assert seen >= 4
