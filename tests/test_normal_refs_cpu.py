"""CPU: the references of generation.normal (tests/normal_refs.py) against each other, on the inputs tests/test_gpu_normal.py feeds the kernel.
  * the float32 numpy restatement against float64: D, the largest deviation of normal_f32, printed and written to profiles/normal_parity.txt;
  * the u8 boundary condition of the GPU test: at most 1 % of the pixels have a pre-truncation value within 512 D of an integer (127.5, the scale
    of the u8 image, times the 4 D the kernel's normal_f32 may deviate), so the +-1 allowance there covers few pixels and the rest must be exact;
  * the matte reference with sigma, and the formula's exact cases."""
import os

import numpy as np

import normal_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_f32_demo_order_against_f64_and_D():
    cases, D = R.parity()
    lines = ["generation.normal: numpy float32 in the demo's operation order against float64, on the inputs of tests/test_gpu_normal.py",
             "(tests/test_normal_refs_cpu.py writes this file; D is what tests/test_gpu_normal.py's tolerances are multiples of)"]
    for (H, W), c in cases.items():
        d = float(np.abs(c["f32"]["normal"].astype(np.float64) - c["f64"]["normal"]).max())
        da = float(np.abs(c["f32"]["ambient"].astype(np.float64) - c["f64"]["ambient"]).max())
        lines.append(f"{R.N_FRAMES} x {H} x {W}: max|normal_f32 - normal_f64| = {d:.3e}   max|ambient_f32 - ambient_f64| = {da:.3e}")
        assert np.isfinite(c["f32"]["normal"]).all() and np.isfinite(c["f64"]["normal"]).all()
        assert da <= 3 * 2.0 ** -24                         # three rounded sums of values in [0, 4]; * 0.25 is exact
    lines.append(f"D = {D:.3e}")
    print("\n".join(lines))
    # every operation of the formula is a few f32 roundings of values of magnitude <= 4, and s -> s^5 multiplies an error by at most 5
    assert 0 < D < 2e-5
    with open(os.path.join(ROOT, "profiles", "normal_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_u8_boundary_condition_of_the_inputs():
    cases, D = R.parity()
    near = total = 0
    for (H, W), c in cases.items():
        m = R.near_integer(c["f64"]["y"], 512 * D)
        print(f"{H} x {W}: {int(m.sum())} of {m.size} pixels within 512 D = {512 * D:.3e} of an integer")
        near, total = near + int(m.sum()), total + m.size
    assert total == sum(R.N_FRAMES * H * W for H, W in R.SHAPES)
    assert near <= 0.01 * total, (near, total)


def test_inputs_cover_the_edge_cases():
    for H, W in R.SHAPES:
        rel, alpha = R.kernel_inputs(H, W)
        assert all(x.dtype == F32 and x.shape == (R.N_FRAMES, 3, H, W) for x in rel) and alpha.shape == (R.N_FRAMES, 1, H, W)
        assert all((x < 0).any() and (x > 1).any() for x in rel) and sum(int(np.isnan(x).sum()) for x in rel) == 1
        assert (alpha == 0).any() and (alpha == 1).any() and int(np.isnan(alpha).sum()) == 1
    assert (5 * 7) % 4 != 0 and (64 * 64) % 4 == 0 and R.N_FRAMES * 64 * 64 // 4 > 256           # both paths; more than one block


def test_formula_exact_cases():
    g = np.random.default_rng(0)
    x = g.random((1, 3, 4, 5), dtype=F32)
    a = g.random((1, 1, 4, 5), dtype=F32)
    for ref in (R.normal_f64, R.normal_f32):
        r = ref(x, x, x, x, a)["normal"]                                            # no direction differs: the normal points at the viewer
        assert np.abs(r[:, :2]).max() == 0 and np.abs(r[:, 2] - 1).max() < 1e-6
        z = np.zeros_like(x)
        r = ref(z, z, z, z, None)["normal"]                                         # black frames: e / e - 1 = 0
        assert np.abs(r[:, :2]).max() == 0 and np.abs(r[:, 2] - 1).max() == 0
    rel = [g.random((1, 3, 4, 5), dtype=F32) for _ in range(4)]
    r0 = R.normal_f64(*rel, np.zeros_like(a))
    assert np.array_equal(np.trunc(r0["y"]), np.broadcast_to(np.array([127.0, 127.0, 255.0]), r0["y"].shape))      # alpha 0: (127, 127, 255)
    assert np.array_equal(R.normal_f64(*rel, None)["y"], R.normal_f64(*rel, np.ones_like(a))["y"])
    # a light from the right makes u positive, one from the top makes v positive
    lo, hi = np.full_like(x, 0.25), np.full_like(x, 0.75)
    mid = np.full_like(x, 0.5)
    r = R.normal_f64(lo, hi, mid, mid, None)["normal"]
    assert (r[:, 0] > 0).all() and np.abs(r[:, 1]).max() == 0
    r = R.normal_f64(mid, mid, lo, hi, None)["normal"]
    assert (r[:, 1] > 0).all() and np.abs(r[:, 0]).max() == 0
    # the bound the kernel rests on: u^2 + v^2 + h^2 >= 0.30 whatever u, v
    rr = np.linspace(0.0, 1.0, 100001)
    assert (rr + (1.0 - rr) ** 10).min() >= 0.30


def test_matte_reference_with_sigma():
    import fbc_refs
    g = np.random.default_rng(1)
    f, a = g.random((2, 3, 5, 7), dtype=F32), g.random((2, 1, 5, 7), dtype=F32)
    assert np.array_equal(R.matte_q(f, a, 0.0), fbc_refs.matte_q(f, a))             # sigma 0: the plain matte
    us = [0, 126, 127, 128, 255]
    ff = (np.array(us, dtype=F32) / F32(255.0)).astype(F32)
    assert R.matte_q(ff, 0.0, 16.0).tolist() == [127] * 5
    assert R.matte_q(ff, 1.0, 16.0).tolist() == [16, 142, 143, 144, 255]            # u + 16, clamped
    assert R.matte_q(ff, 0.5, 16.0).tolist() == [71, 134, 135, 135, 199]            # 127 + (u - 111)/2 truncated: 71.5, 134.5, 135, 135.5, 199
    assert R.matte_q(ff, np.nan, 16.0).tolist() == [0] * 5                          # NaN -> 0
