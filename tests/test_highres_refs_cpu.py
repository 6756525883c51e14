"""CPU: tests/highres_refs.py, the numpy restatement the GPU tests of the highres pass compare against, pinned to PIL itself bit for bit
(Image.resize with Image.LANCZOS), and the host table of the library (tcl_resize_lanczos_table: f64 with the C library's sin) pinned to the restatement."""
import ctypes
import os

import numpy as np
import pytest

import highres_refs as R


def _pil_resize(img, h_out, w_out):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(f).resize((w_out, h_out), Image.LANCZOS)) for f in img])


@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}->{c[1][0]}x{c[1][1]}")
def test_resize_restatement_is_pil(case, kind):
    (h, w), (ho, wo) = case
    img = R.content(kind, 2, h, w, seed=h * 1000 + w)
    got, want = R.resize_lanczos(img, ho, wo), _pil_resize(img, ho, wo)
    assert got.shape == want.shape == (2, ho, wo, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ from PIL"


def test_contents_reach_both_clips():
    """The checkerboard makes Lanczos overshoot: the restatement must have clipped at both ends somewhere (else those cases pin nothing)."""
    img = R.content("checker", 1, 40, 72)
    bounds, taps = R.lanczos_table(72, 128)
    acc = [int((taps[o, :c].astype(np.int64) * img[0, 0, lo:lo + c, 0]).sum() + (1 << 21)) >> 22 for o, (lo, c) in enumerate(bounds)]
    assert min(acc) < 0 and max(acc) > 255


def test_unchanged_axis_is_not_resampled():
    img = R.content("random", 1, 64, 80, seed=4)
    assert R._resample(img, 1, 64) is img
    assert np.array_equal(R.resize_lanczos(img, 64, 80), img)


def test_table_shape_and_normalisation():
    for n_in, n_out, ksize in ((40, 64, 7), (16, 64, 7), (72, 64, 9), (96, 64, 11), (128, 64, 13)):
        b, k = R.lanczos_table(n_in, n_out)
        assert k.shape == (n_out, ksize) and b.shape == (n_out, 2)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] >= 1).all()
        assert (np.diff(b[:, 0]) >= 0).all()
        assert np.abs(k.sum(1) - (1 << 22)).max() <= ksize              # each tap is rounded on its own
        for o in range(n_out):
            assert not k[o, b[o, 1]:].any()


def test_quantise_restatement():
    v = R.quantise_probes()
    u = R.frames_to_u8(np.broadcast_to(v[None, None, None, :], (1, 3, 1, v.size)))
    assert u.shape == (1, 1, v.size, 3) and u.dtype == np.uint8
    want = [int(min(max(float(np.float32(255.0) * x), 0.0), 255.0)) for x in v]
    assert u[0, 0, :, 1].tolist() == want
    k = np.arange(256)
    assert (u[0, 0, :256, 0] >= k - 1).all() and (u[0, 0, :256, 0] <= k).all()      # fl32(255 * fl32(k/255)) is k or just below it
    assert u[0, 0, 768, 0] == 0                                                    # -0.0


def test_library_table_matches_restatement():
    """tcl_resize_lanczos_table is host code: it runs without a GPU.  One flipped 22-bit tap would break bit-identity with PIL."""
    import __graft_entry__ as g
    from tc_light_amd.lib import LIB_PATH
    if not os.path.exists(LIB_PATH):
        g.build()
    dll = ctypes.CDLL(LIB_PATH)
    dll.tcl_resize_lanczos_table_ints.restype = ctypes.c_size_t
    dll.tcl_resize_lanczos_table.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    sizes = [(a, b) for (h, w), (ho, wo) in R.CASES for a, b in ((h, ho), (w, wo)) if a != b] + [(720, 1088), (1280, 1920), (1088, 720), (99, 64)]
    for n_in, n_out in sizes:
        want = R.table_ints(n_in, n_out)
        assert dll.tcl_resize_lanczos_table_ints(n_in, n_out) == want.size
        got = np.full(want.size + 4, -77, np.int32)
        assert dll.tcl_resize_lanczos_table(n_in, n_out, got.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(got[:-4], want) and (got[-4:] == -77).all(), (n_in, n_out)
    assert dll.tcl_resize_lanczos_table_ints(64, 64) == 0 and dll.tcl_resize_lanczos_table_ints(15, 64) == 0
    assert dll.tcl_resize_lanczos_table_ints(129, 64) == 0 and dll.tcl_resize_lanczos_table_ints(0, 64) == 0
    buf = np.zeros(8, np.int32)
    assert dll.tcl_resize_lanczos_table(64, 64, buf.ctypes.data_as(ctypes.c_void_p)) == 1
    assert dll.tcl_resize_lanczos_table(40, 64, None) == 1
