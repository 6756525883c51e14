"""CPU: light-follow's float64 restatement (tests/lightfit_refs.py) recovers a planted plane, its host side (tc_light_amd/lightfit.py) resolves the
wanted angles and solves as the restatement does, and the frames that have no estimate are counted as such.  Nothing here needs the kernel."""
import math

import numpy as np
import pytest

import lightfit_refs as R
from tc_light_amd import lightfit


@pytest.fixture(scope="module")
def planted():
    E, S = R.planted(len(R.ANGLES), 37, 53, R.ANGLES, seed=5)
    return E, S, R.sums_ref(E, S)


def test_reference_recovers_the_planted_plane(planted):
    """A condition on the INPUTS the GPU test uses: with amplitude R.AMPLITUDE = 0.3 the f64 reference alone lands within 2 degrees of the planted
    angle at 0, 37, 90, 200 and 315 degrees on 37x53 frames (it lands within 0.05), and its contrast is the amplitude to a few per cent."""
    E, S, (sums, bound) = planted
    assert sums.shape == (5, 10) and (sums[:, 0] == 37 * 53).all(), "nothing of the planted frames may clip"
    for row, want in zip(sums, R.ANGLES):
        ok, ang, con, r2 = R.solve_ref(row)
        print(f"planted {want}: estimated {ang:.4f}, contrast {con:.4f}, R^2 {r2:.4f}")
        assert ok and R.angle_diff(ang, want) <= 2.0
        assert abs(con - R.AMPLITUDE) <= 0.05 * R.AMPLITUDE and 0.9 < r2 <= 1.0
    follow, contrast = R.figures_ref(sums, R.ANGLES)
    assert follow > math.cos(math.radians(2.0)) and abs(contrast - R.AMPLITUDE) <= 0.05 * R.AMPLITUDE
    assert abs(R.figures_ref(sums, [a + 180.0 for a in R.ANGLES])[0] + follow) < 1e-12, "the opposite light scores the negative"


def test_bounds_are_small_and_the_implied_angle_error_is_tiny(planted):
    _, _, (sums, bound) = planted
    assert (bound[:, 0] == 0).all() and (bound[:, 1:] > 0).all()
    assert (bound[:, 1:] <= 1e-5 * 37 * 53 * 40).all()
    worst = max(R.angle_bound_deg(row, b) for row, b in zip(sums, bound))
    print(f"angle error the sum bounds allow at 37x53: {worst:.3e} degrees")
    assert worst < 0.05


def test_host_solve_matches_the_restatement(planted):
    _, _, (sums, _) = planted
    follow, contrast, frames = lightfit.figures(sums, R.ANGLES)
    rf, rc = R.figures_ref(sums, R.ANGLES)
    assert abs(follow - rf) <= 1e-12 and abs(contrast - rc) <= 1e-12
    for f, row, want in zip(frames, sums, R.ANGLES):
        ok, ang, con, r2 = R.solve_ref(row)
        assert f["estimate"] and ok and f["wanted"] == want
        assert R.angle_diff(f["angle"], ang) <= 1e-9 and abs(f["contrast"] - con) <= 1e-12 and abs(f["r2"] - r2) <= 1e-9
        assert 0.0 <= f["angle"] < 360.0


def test_wanted_angles_from_a_path_use_the_runs_interpolation():
    from tc_light_amd import hostlogic
    cfg = {"generation": {"light_path": [[0, 0], [0.5, 90], [1, 450]]}}
    got = lightfit.wanted_angles(cfg, 5)
    assert got == [0.0, 45.0, 90.0, 270.0, 450.0]
    assert got == hostlogic.light_angles(hostlogic.check_light_path(cfg["generation"]["light_path"]), hostlogic.light_positions(5))
    assert lightfit.wanted_angles({"generation": {"light_path": [[0, 30]]}}, 3) == [30.0] * 3
    assert lightfit.wanted_angles(cfg, 1) == [0.0]


@pytest.mark.parametrize("side", sorted(R.SIDE_ANGLE))
def test_wanted_angles_from_a_side(side):
    assert lightfit.wanted_angles({"generation": {"init_latent": side}}, 4) == [R.SIDE_ANGLE[side]] * 4
    assert lightfit.wanted_angles({"generation": {"iclight_model": "fbc", "bg_source": side}}, 2) == [R.SIDE_ANGLE[side]] * 2
    with pytest.raises(ValueError, match="bg_source"):                      # a ramp counts under fbc only: fc never reads bg_source
        lightfit.wanted_angles({"generation": {"bg_source": side}}, 2)


@pytest.mark.parametrize("gen", [{}, {"init_latent": "none"}, {"init_latent": "source"}, {"iclight_model": "fbc", "bg_source": "grey"},
                                 {"iclight_model": "fbc", "bg_source": "upload"}, {"light_path": None}])
def test_wanted_angles_refusal_names_the_keys(gen):
    with pytest.raises(ValueError) as e:
        lightfit.wanted_angles({"generation": gen}, 3)
    for key in ("generation.light_path", "generation.init_latent", "generation.bg_source", "--light_path"):
        assert key in str(e.value)
    with pytest.raises(ValueError):
        lightfit.wanted_angles({}, 3)


def test_light_path_override_wins_and_is_checked():
    cfg = {"generation": {"init_latent": "left", "light_path": [[0, 10]]}}
    assert lightfit.wanted_angles(cfg, 3, light_path=[[0, 0], [1, 180]]) == [0.0, 90.0, 180.0]
    assert lightfit.wanted_angles({}, 2, light_path=[[0, 0], [1, 180]]) == [0.0, 180.0]
    with pytest.raises(ValueError, match="light_path"):
        lightfit.wanted_angles({}, 3, light_path=[[0.5, 0]])
    with pytest.raises(ValueError, match="light_path"):
        lightfit.wanted_angles({}, 3, light_path="left")


def _no_estimate(E, S, n):
    sums, _ = R.sums_ref(E, S)
    follow, contrast, frames = lightfit.figures(sums, [0.0] * n)
    assert follow == 0.0 and contrast == 0.0
    for f, row in zip(frames, sums):
        assert R.solve_ref(row)[0] is False
        assert f["estimate"] is False and f["cos"] == 0.0 and f["angle"] is None and f["contrast"] is None and f["r2"] is None
    return sums


def test_no_estimate_all_pixels_clipped():
    S = np.full((2, 3, 9, 11), 128, np.uint8)
    E = np.stack([np.full((3, 9, 11), 255, np.uint8), np.zeros((3, 9, 11), np.uint8)])
    sums = _no_estimate(E, S, 2)
    assert (sums == 0).all()
    assert (_no_estimate(S, E, 2) == 0).all()                               # a clipped source drops the pixel too
    edge = np.full((1, 3, 4, 4), 2, np.uint8), np.full((1, 3, 4, 4), 253, np.uint8)      # 2 and 253 are inside the interval
    assert R.sums_ref(*edge)[0][0, 0] == 16
    edge = np.full((1, 3, 4, 4), 1, np.uint8), np.full((1, 3, 4, 4), 128, np.uint8)
    assert R.sums_ref(*edge)[0][0, 0] == 0


def test_no_estimate_one_pixel_frame():
    E, S = np.full((1, 3, 1, 1), 100, np.uint8), np.full((1, 3, 1, 1), 80, np.uint8)
    sums = _no_estimate(E, S, 1)
    assert sums[0, 0] == 1.0 and sums[0, 1] == 0.0 and sums[0, 2] == 0.0   # one pixel, at the centre
    line_e, line_s = R.planted(1, 1, 64, [0.0], seed=2)                     # a single row: v is 0 everywhere, the system is singular
    _no_estimate(line_e, line_s, 1)


def test_no_estimate_when_edit_equals_source():
    _, S = R.planted(2, 21, 34, [0.0, 90.0], seed=3)
    sums = _no_estimate(S, S, 2)
    assert (sums[:, 0] == 21 * 34).all() and (sums[:, 6:] == 0).all()


def test_a_mix_of_frames_counts_the_missing_ones_as_zero():
    E, S = R.planted(2, 37, 53, [0.0, 0.0], seed=7)
    E[1] = 255
    follow, contrast, frames = lightfit.figures(R.sums_ref(E, S)[0], [0.0, 0.0])
    assert [f["estimate"] for f in frames] == [True, False]
    assert abs(follow - frames[0]["cos"] / 2) < 1e-15 and abs(contrast - frames[0]["contrast"] / 2) < 1e-15
