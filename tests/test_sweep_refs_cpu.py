"""CPU: the two properties of the angle ramp's reference (tests/sweep_refs.py) that the routing rule of Generator.light_ramps rests on.
  * At 0 / 90 / 180 / 270 the formula is, in real arithmetic, the np.linspace rule of tcl_light_gradient_f32 / tcl_bg_ramp_f32; the roundings differ, so
    the two may disagree by one uint8 level at isolated pixels, never by more, and agree on the two end pixels.
  * Away from the axes the levels never rise along (c, s).
Where the ramp's axis has a single sample (W == 1 at 0 / 180, H == 1 at 90 / 270, so R == 0) np.linspace(start, stop, 1) keeps `start`; the formula's
rule for R == 0, t = ((|c| + |s|) + (c + s)) / (2(|c| + |s|)), is exactly 1 at 0 / 90 and 0 at 180 / 270, the same level.  Measured: at all five sizes
and both level pairs no pixel differs."""
import numpy as np
import pytest

import sweep_refs as R


@pytest.mark.parametrize("H,W", R.SIZES)
def test_axis_angles_equal_linspace_within_one_level(H, W):
    worst, bad_ends = 0, []
    for hi, lo in R.LEVELS:
        for angle in (0.0, 90.0, 180.0, 270.0):
            (c, s), = R.dirs([angle])
            got = R.ramp_u8(c, s, H, W, hi, lo).astype(np.int64)
            want = R.linspace_u8(angle, H, W, hi, lo).astype(np.int64)
            diff = np.abs(got - want)
            print(f"[angle ramp vs linspace] {H}x{W} levels ({hi}, {lo}) angle {angle:g}: max |difference| = {diff.max()}, "
                  f"{int((diff > 0).sum())} of {H * W} pixels differ")
            worst = max(worst, int(diff.max()))
            if diff.flat[0] != 0 or diff.flat[-1] != 0:
                bad_ends.append((hi, lo, angle))
    assert worst <= 1, worst
    assert not bad_ends, bad_ends


@pytest.mark.parametrize("H,W", R.SIZES)
@pytest.mark.parametrize("angle", [37.5, 135.0, 200.25])
def test_levels_never_rise_along_the_direction(H, W, angle):
    """Pixels ordered by d = px*c + py*s (the coordinate along (c, s)): the level is non-increasing, and pixels of equal d share a level."""
    (c, s), = R.dirs([angle])
    d, _ = R.ramp_d(c, s, H, W)
    for hi, lo in R.LEVELS:
        u = R.ramp_u8(c, s, H, W, hi, lo).astype(np.int64)
        order = np.argsort(d, axis=None, kind="stable")
        ds, us = d.flat[order], u.flat[order]
        rising = np.diff(us) > 0
        assert not (rising & (np.diff(ds) > 0)).any()               # a level that rises where d rises
        assert not (rising & (np.diff(ds) == 0)).any()              # equal d, different levels
        assert us[0] <= hi and us[-1] >= lo and (H * W == 1 or us[0] >= us[-1])
        # along the rows and the columns on their own, by the sign of c and s
        if W > 1:
            assert (np.diff(u, axis=1) * np.sign(c) <= 0).all()
        if H > 1:
            assert (np.diff(u, axis=0) * np.sign(s) <= 0).all()


def test_end_levels_and_the_convention():
    """0 = left (bright at x = 0), 90 = top (bright at y = 0), 180 = right, 270 = bottom; at a general angle hi sits at the corner nearest the light."""
    H, W = 17, 33
    for hi, lo in R.LEVELS:
        for angle, bright, dark in ((0.0, (8, 0), (8, 32)), (90.0, (0, 16), (16, 16)), (180.0, (8, 32), (8, 0)), (270.0, (16, 16), (0, 16)),
                                    (37.5, (0, 0), (16, 32)), (135.0, (0, 32), (16, 0)), (200.25, (16, 32), (0, 0))):
            (c, s), = R.dirs([angle])
            u = R.ramp_u8(c, s, H, W, hi, lo)
            assert u[bright] == hi == u.max() and u[dark] == lo == u.min(), (angle, hi, lo)
