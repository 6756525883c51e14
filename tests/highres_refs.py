"""numpy restatements for the highres pass (csrc/resize.hip): the quantise step and PIL's LANCZOS resize in its own integer arithmetic.
tests/test_highres_refs_cpu.py pins `resize_lanczos` to PIL itself, bit for bit; the GPU tests then compare the kernels with these functions.

PIL's ImagingResample (Resample.c) per axis: scale = in/out, filterscale = max(scale, 1), support = 3*filterscale, ksize = 2*ceil(support) + 1; per
output index the window int(center -/+ support + 0.5) clamped to the image, f64 Lanczos-3 weights normalised by their sum, rounded half away from
zero to 22-bit fixed point; the accumulator starts at 1 << 21, is shifted right by 22 and clipped to u8; horizontal pass first, clipped to u8 before
the vertical pass; an axis whose size does not change is not resampled."""
import math

import numpy as np

PBITS = 32 - 8 - 2

# (in H, in W) -> (out H, out W): the cases of the issue's table
CASES = [((40, 72), (64, 128)),       # non-integer up-scale, different per axis
         ((64, 80), (64, 128)),       # one axis unchanged: that pass is skipped
         ((72, 136), (64, 128)),      # slight down-scale (the 64-rounding can shrink)
         ((33, 47), (64, 64)),        # odd sizes, windows cut at every border
         ((128, 96), (64, 64)),       # ratios 2 and 1.5
         ((16, 16), (64, 64))]        # ratio 0.25
CONTENTS = ("random", "zeros", "full", "checker")


def content(kind, n, h, w, seed=0):
    """[n,h,w,3] u8: random, all 0, all 255, or a 1-pixel checkerboard (Lanczos overshoot clips at both ends)."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((n, h, w, 3), np.uint8)
    if kind == "full":
        return np.full((n, h, w, 3), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        out[i] = (board if i % 2 == 0 else 255 - board)[..., None]
    return out


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def lanczos_table(n_in, n_out):
    """-> (bounds [n_out,2] int32 = (first input index, tap count), taps [n_out,ksize] int32), precompute_coeffs + normalize_coeffs_8bpc."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, taps = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        taps[xx, :xmax] = [int(-0.5 + v * (1 << PBITS)) if v < 0 else int(0.5 + v * (1 << PBITS)) for v in w]
        bounds[xx] = xmin, xmax
    return bounds, taps


def table_ints(n_in, n_out):
    """The flat table tcl_resize_lanczos_table writes: bounds, then taps."""
    b, k = lanczos_table(n_in, n_out)
    return np.concatenate([b.reshape(-1), k.reshape(-1)]).astype(np.int32)


def _resample(img, axis, n_out):
    """One pass over `axis` (1 = rows / vertical, 2 = columns / horizontal) of img [N,H,W,3] u8."""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    bounds, taps = lanczos_table(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for o in range(n_out):
        lo, cnt = bounds[o]
        acc = np.tensordot(taps[o, :cnt].astype(np.int64), src[lo:lo + cnt], axes=(0, 0)) + (1 << (PBITS - 1))
        out[o] = np.clip(acc >> PBITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_lanczos(img, h_out, w_out):
    """[N,H,W,3] u8 -> [N,h_out,w_out,3] u8 = PIL.Image.resize((w_out, h_out), Image.LANCZOS) of every frame."""
    return _resample(_resample(np.asarray(img), 2, w_out), 1, h_out)


def frames_to_u8(p):
    """tcl_frames_to_u8: [N,3,H,W] f32 -> [N,H,W,3] u8, u = trunc(clamp(fl32(255 * p), 0, 255))."""
    p = np.asarray(p, np.float32)
    s = np.float32(255.0) * p
    u = np.clip(s, np.float32(0), np.float32(255)).astype(np.uint8)
    return np.ascontiguousarray(u.transpose(0, 2, 3, 1))


def quantise_probes():
    """f32 values around every k/255 (the value and one ulp either side), values below 0 and above 1, and -0.0."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    v = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                        np.array([-0.0, -1e-8, -0.5, -3.0, 1.0000001, 1.002, 1.5, 7.0, 1e30, -1e30], np.float32)]).astype(np.float32)
    return v
