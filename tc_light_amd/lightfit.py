"""light-follow and light-contrast (evaluate.py --light): does the relit light obey its light_path?

The relit clip E is compared with its source S frame by frame: the log ratio of their luminances, r = log((Ye + 1/255) / (Ys + 1/255)), is fitted by
a plane r ~ a + gx*u + gy*v over the unclipped pixels (u, v in (-1, 1), the pixel centres), and the plane's gradient says where the light comes
from.  The ten weighted sums per frame come from tcl_light_fit_u8 (csrc/lightfit.hip; the definition is in include/tclight_hip.h); the 3x3 normal
equations are solved here in float64.

  angle     atan2(-gy, -gx) in degrees mod 360, in light_path's convention: the side the light comes FROM (0 left, 90 top, 180 right, 270 bottom)
  contrast  hypot(gx, gy)
  R^2       1 - SS_res / SS_tot, both from the sums (Swrr among them)
A frame has no estimate when Sw < 3, when the system is singular or when the contrast is 0; it then counts with cosine 0.
  light-follow    mean over the frames of cos(angle - wanted angle)
  light-contrast  mean over the frames of the contrast (0 where there is no estimate)
The wanted angle of a frame comes from the run's config (`wanted_angles`): generation.light_path through hostlogic's keyframe interpolation, else the
constant side of generation.init_latent or of an fbc ramp generation.bg_source.
"""
import math

import numpy as np
import torch

from . import hostlogic
from .lib import check, lib, stream

SUMS = ("w", "wu", "wv", "wuu", "wuv", "wvv", "wr", "wru", "wrv", "wrr")
SINGULAR_RTOL = 1e-12         # det <= SINGULAR_RTOL * Sw * Swuu * Swvv (Hadamard's bound on the determinant of the Gram matrix): singular
KEYS_LOOKED_FOR = "generation.light_path, generation.init_latent (left | right | top | bottom), generation.bg_source (left | right | top | bottom, under " \
                  "generation.iclight_model fbc)"


def light_sums(edit_nchw, source_nchw):
    """edit / source uint8 [N,3,H,W] on the device, contiguous -> sums f64 [N,10] on the device (the order of SUMS)."""
    e, s = check(edit_nchw, torch.uint8), check(source_nchw, torch.uint8)
    if e.dim() != 4 or e.shape[1] != 3 or e.shape != s.shape:
        raise ValueError(f"light_sums takes two uint8 [N,3,H,W] tensors of one shape, got {tuple(e.shape)} / {tuple(s.shape)}")
    N, _, H, W = e.shape
    L = lib()
    nbytes = L.tcl_light_fit_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise ValueError(f"light_sums: N in 1..65535, H, W > 0 and H*W < 2^31, got N {N}, {H}x{W}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    out = torch.empty(N, len(SUMS), dtype=torch.float64, device=e.device)
    L.tcl_light_fit_u8(e, s, N, H, W, out, ws, stream())
    return out


def solve_frame(sums):
    """The ten sums of one frame (f64) -> {"estimate": bool, "angle", "contrast", "r2"}; the last three are None without an estimate."""
    sw, swu, swv, swuu, swuv, swvv, swr, swru, swrv, swrr = (float(v) for v in sums)
    none = {"estimate": False, "angle": None, "contrast": None, "r2": None}
    if not sw >= 3.0:
        return none
    A = np.array([[sw, swu, swv], [swu, swuu, swuv], [swv, swuv, swvv]], dtype=np.float64)
    b = np.array([swr, swru, swrv], dtype=np.float64)
    det = float(np.linalg.det(A))
    if not det > SINGULAR_RTOL * sw * swuu * swvv:
        return none
    a, gx, gy = (float(v) for v in np.linalg.solve(A, b))
    contrast = math.hypot(gx, gy)
    if not (math.isfinite(contrast) and contrast > 0.0):
        return none
    angle = math.degrees(math.atan2(-gy, -gx)) % 360.0
    ss_res = swrr - (a * swr + gx * swru + gy * swrv)         # the normal equations' identity for the residual of the fit
    ss_tot = swrr - swr * swr / sw
    r2 = 1.0 - ss_res / ss_tot if ss_tot > 0.0 else 0.0
    return {"estimate": True, "angle": 0.0 if angle >= 360.0 else angle, "contrast": contrast, "r2": r2}


def figures(sums, wanted):
    """sums [N,10] f64 (numpy), wanted: N angles in degrees -> (light-follow, light-contrast, per-frame list of dicts: frame, wanted, angle,
    contrast, r2, estimate, cos)."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != len(SUMS) or len(wanted) != sums.shape[0] or sums.shape[0] < 1:
        raise ValueError(f"figures takes sums [N,{len(SUMS)}] and N wanted angles, got {sums.shape} and {len(wanted)}")
    frames = []
    for i, (row, want) in enumerate(zip(sums, wanted)):
        fit = solve_frame(row)
        fit["cos"] = math.cos(math.radians(fit["angle"] - float(want))) if fit["estimate"] else 0.0
        frames.append({"frame": i, "wanted": float(want), **fit})
    follow = float(np.mean([f["cos"] for f in frames]))
    contrast = float(np.mean([f["contrast"] if f["estimate"] else 0.0 for f in frames]))
    return follow, contrast, frames


def wanted_angles(config, n_frames, light_path=None):
    """The angle each of the run's n_frames should be lit from, in degrees.  `light_path` (--light_path, keyframes [[pos, angle_deg], ...]) wins;
    else the config's generation.light_path -- both through hostlogic.check_light_path and the run's own interpolation (light_positions /
    light_angles); else the constant side of generation.init_latent, or of generation.bg_source under generation.iclight_model fbc: left 0, top 90,
    right 180, bottom 270.  A run that names none of them is refused with a ValueError listing the keys."""
    gen = (config.get("generation") if hasattr(config, "get") else None) or {}
    path = light_path if light_path is not None else gen.get("light_path")
    if path is not None:
        keys = hostlogic.check_light_path(path)
        return hostlogic.light_angles(keys, hostlogic.light_positions(n_frames))
    side = str(gen.get("init_latent") or "none").lower()
    if side not in hostlogic.LIGHT_AXIS_SIDES and str(gen.get("iclight_model") or "fc").lower() == "fbc":
        side = str(gen.get("bg_source") or "upload").lower()
    if side not in hostlogic.LIGHT_AXIS_SIDES:
        raise ValueError(f"--light: the run's config names no light direction; looked for {KEYS_LOOKED_FOR}, or pass --light_path")
    return [90.0 * hostlogic.LIGHT_AXIS_SIDES.index(side)] * n_frames
