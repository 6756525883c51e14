"""Restatements for the tests of the light-direction / strength start (generation.init_latent, init_strength), written from the recipe's formulas:
the img2img schedule, the demo's gradient image and the add_noise start in numpy f32.  TEST INFRASTRUCTURE: nothing here imports the engine."""
import numpy as np

SIDES = ("left", "right", "top", "bottom")       # the order of TCL_LIGHT_* in include/tclight_hip.h


def schedule(n, s):
    """(scheduler steps, begin index, steps executed): n_sched = round(n / s), run = min(int(n_sched * s), n_sched), begin = n_sched - run."""
    n_sched = round(n / s)
    run = min(int(n_sched * s), n_sched)
    return n_sched, n_sched - run, run


def gradient_u8(side, H, W):
    """The uint8 plane [H,W]: np.linspace(255, 0, W) for left, (0, 255, W) for right, the same over H for top / bottom, cast by truncation."""
    a, b = (255, 0) if side in ("left", "top") else (0, 255)
    if side in ("left", "right"):
        plane = np.tile(np.linspace(a, b, W), (H, 1))
    else:
        plane = np.tile(np.linspace(a, b, H)[:, None], (1, W))
    return plane.astype(np.uint8)


def gradient_image(side, H, W):
    """[3,H,W] f32 = u/254 (one f32 division): the [0,1]-convention image whose 2x - 1 is the u/127 - 1 the VAE is to see."""
    u = gradient_u8(side, H, W)
    return np.broadcast_to(u.astype(np.float32) / np.float32(254), (3, H, W)).copy()


def start(x0, z, alpha, sigma_t):
    """f16(fl32(fl32(alpha*x0) + fl32(sigma_t*z))): x0 f16 and z f32 broadcast against each other over the frames, alpha / sigma_t rounded to f32 once."""
    a = np.float32(alpha) * x0.astype(np.float32)
    b = np.float32(sigma_t) * z.astype(np.float32)
    assert a.dtype == np.float32 and b.dtype == np.float32
    return (a + b).astype(np.float16)
