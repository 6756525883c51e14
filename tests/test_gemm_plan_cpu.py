"""Which tile a GEMM / conv3x3 shape gets is decided on the host (csrc/gemm.hip: choose) and decides its speed; every tile yields the same bits, so
no numerical test notices a shape that is silently re-routed.  tcl_gemm_plan / tcl_conv3x3_plan ask that choice without a GPU; this test pins the
answer for every shape of the committed tile table, and for the paths around the table, to tests/golden/gemm_plan_gfx950.txt."""
import os
import shutil

import pytest
import torch

from tc_light_amd import lib as libmod
from tc_light_amd.unet import GEMM_TABLE

EXPECT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_gfx950.txt")
WS_BYTES = 96 << 20
# the stride-2, pad-0 and up-sampled convolutions of test_gpu_kernels.py::test_gemm8q_epilogues_and_tails_equal_tiled_kernels:
# (B, Hin, Win, Cin, Cout, stride, pad, Hup, Wup, act), has a residual
CONV_TAILS = [((3, 46, 30, 640, 640, 2, 1, 0, 0, 0), 0), ((3, 12, 20, 640, 1280, 1, 1, 23, 40, 0), 0), ((2, 10, 16, 256, 256, 1, 1, 20, 32, 0), 1),
              ((40, 3, 6, 640, 640, 1, 1, 3, 12, 0), 0), ((2, 40, 56, 256, 256, 2, 0, 0, 0, 0), 0), ((5, 23, 30, 320, 640, 1, 1, 0, 0, 1), 1),
              ((2, 44, 60, 128, 128, 2, 0, 0, 0, 0), 0)]


def _dense(M, N, K, act=0, resid=0, ldc=None):
    return ("dense", (M, N, K, K, K, ldc if ldc else (N // 2 if act == 2 else N), N, act), resid)


def sections():
    """[(name, [(forced (cfg, splits) or None, kind, args, resid)])]: the problems, in the order of the expectation file."""
    rows = [tuple(int(v) for v in ln.split()) for ln in open(GEMM_TABLE) if ln[0] not in "#!" and ln.strip()]
    dense = [r for r in rows if r[0] == 0]
    in_table = {r[1:6] for r in dense}
    auto = lambda ps: [(None,) + p for p in ps]
    out = [("table, dense", auto(_dense(M, N, K, act, hasr) for _, M, N, K, act, hasr, *_ in dense))]
    conv = []
    for cv, M, N, K, act, hasr, Hin, Win, Cin, stride, Hup, _cfg in rows:
        if cv == 1 and stride == 1 and Hup == Hin:           # pad 1, no up-sampling: Hout x Wout = Hin x Win, so the batch follows from M
            assert M % (Hin * Win) == 0 and K == 9 * Cin
            conv.append(("conv", (M // (Hin * Win), Hin, Win, Cin, N, 1, 1, Hin, Win, act), hasr))
    out.append(("table, conv stride 1", auto(conv)))
    out.append(("conv stride 2 / pad 0 / up-sampled", auto(("conv", a, r) for a, r in CONV_TAILS)))
    for name, num in (("dense, M x 1.7 (nearest-M twin)", 17), ("dense, M x 3 (past the twin bound)", 30)):
        out.append((name, auto(_dense(M * num // 10, N, K, act, hasr) for _, M, N, K, act, hasr, *_ in dense
                               if (M * num // 10, N, K, act, hasr) not in in_table)))
    # what the vector epilogues cannot store takes the register-staged kernels: N % 8 != 0, ldc % 8 != 0 (narrow and wide N)
    out.append(("register-staged", auto([_dense(1000, 4, 64), _dense(1000, 132, 320), _dense(1000, 1028, 320), _dense(5000, 320, 320, ldc=324),
                                         _dense(5000, 640, 640, resid=1, ldc=644), _dense(300, 1284, 4096)])))
    # K = 320 with the residual in place: N = 352 / 160 leave a partial last weight tile, which the strip kernel must not get
    out.append(("in-place residual", auto([_dense(5000, 352, 320, resid=2), _dense(5000, 160, 320, resid=2), _dense(40000, 640, 320, resid=2)])))
    out.append(("GEGLU arguments", auto([_dense(20000, 2560, 320, act=2), _dense(20000, 2560, 320, act=2, resid=1), _dense(20000, 2592, 320, act=2)])))
    f = lambda cfg, sp, p: ((cfg, sp),) + p
    out.append(("forced", [
        f(1, 4, _dense(2048, 1280, 5120)), f(3, 1, _dense(3000, 192, 640)), f(11, 2, ("conv", (16, 23, 40, 1280, 1280, 1, 1, 0, 0, 1), 1)),
        f(7, 1, _dense(4096, 1280, 1280)), f(8, 1, _dense(2500, 2560, 320, act=2)), f(5, 1, _dense(2500, 2560, 320, act=2)),      # GEGLU: not on 320 columns
        f(6, 1, ("conv", (4, 45, 80, 640, 640, 1, 1, 0, 0, 0), 0)),
        f(9, 1, _dense(1000, 4, 64)), f(10, 1, _dense(1000, 132, 320)), f(10, 1, _dense(2500, 2560, 320, act=2)), f(9, 3, _dense(2500, 2560, 320, act=2)),
        f(12, 1, _dense(20000, 320, 320, resid=1)), f(12, 1, _dense(20000, 320, 640)), f(12, 1, _dense(5000, 352, 320, resid=2)),
        f(12, 1, _dense(5000, 160, 320, resid=2)), f(12, 1, _dense(5000, 352, 320, resid=1)), f(12, 1, _dense(5000, 320, 320, resid=2)),
        f(13, 1, _dense(3000, 1280, 640, act=1)), f(13, 1, _dense(3000, 320, 640)), f(13, 1, _dense(2500, 2560, 320, act=2)),
        f(14, 1, ("conv", (3, 12, 20, 640, 1280, 1, 1, 23, 40, 0), 0)), f(14, 1, ("conv", (3, 12, 20, 640, 1280, 1, 1, 36, 40, 0), 0)),
        f(14, 1, _dense(2500, 2560, 320, act=2)), f(15, 1, _dense(5000, 128, 448, act=1, resid=1)), f(15, 1, _dense(5000, 128, 448, ldc=132)),
        f(16, 1, _dense(4096, 1280, 1280)), f(1, 1, _dense(1000, 4, 64))]))
    return out


def ask(L, kind, args, resid):
    """-> (cfg, splits), or "EINVAL" where the call itself is refused."""
    out = torch.full((2,), -7, dtype=torch.int32)
    try:
        (L.tcl_gemm_plan if kind == "dense" else L.tcl_conv3x3_plan)(*args, resid, out[0:1], out[1:2])
    except RuntimeError as e:
        assert "TCL_EINVAL" in str(e)
        return "EINVAL"
    return tuple(out.tolist())


def run_sections(L, plan):
    """{(workspace, section): [answers]} for the whole list with a (fake, never dereferenced) 96 MiB split-K workspace and without one."""
    got = {}
    try:
        L.tcl_gemm_tune_load(GEMM_TABLE)
        L.tcl_gemm_autotune(2)                                  # table-only: what the table lacks takes the heuristic, nothing is timed
        for ws in (1, 0):
            L.tcl_set_workspace(0x7f0000000000 if ws else 0, WS_BYTES if ws else 0)
            for name, problems in sections():
                res = []
                for forced, kind, args, resid in problems:
                    if forced:
                        L.tcl_gemm_tune(*forced)
                    try:
                        res.append(plan(L, kind, args, resid))
                    finally:
                        if forced:
                            L.tcl_gemm_tune(0, 0)
                got[(ws, name)] = res
    finally:
        L.tcl_gemm_tune(0, 0)
        L.tcl_set_workspace(0, 0)
        L.tcl_gemm_autotune(1)
    return got


def read_expect(path=EXPECT):
    exp, cur = {}, None
    for ln in open(path):
        ln = ln.strip()
        if ln.startswith("== "):
            ws, name = ln[3:].split(" | ")
            cur = exp.setdefault((int(ws[-1]), name), [])
        elif ln and not ln.startswith("#"):
            cur.append("EINVAL" if ln == "EINVAL" else tuple(int(v) for v in ln.split()))
    return exp


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    """A private copy of the built library: its tile cache then holds the committed table and nothing that GPU tests of the same process measured
    (a measured neighbour would change the nearest-M answers), and the modes set here never reach the engine's instance."""
    so = tmp_path_factory.mktemp("gemm_plan") / "libtclight_plan.so"
    shutil.copy(libmod.LIB_PATH, so)
    mp = pytest.MonkeyPatch()
    mp.setattr(libmod, "LIB_PATH", str(so))
    try:
        return libmod._Lib()
    finally:
        mp.undo()


def test_gemm_plan_matches_the_recorded_choice(L):
    """The expectations were recorded from the dispatcher as it was BEFORE choose() was split out of it (a build whose run_cfg recorded its (cfg, splits)
    instead of launching, asked through tcl_gemm_f16 / tcl_conv3x3_f16 with fake operands), not from tcl_gemm_plan."""
    got, exp = run_sections(L, ask), read_expect()
    assert set(got) == set(exp)
    n = 0
    for key, res in got.items():
        assert len(res) == len(exp[key]), key
        probs = dict(sections())[key[1]]
        bad = [(p, g, e) for p, g, e in zip(probs, res, exp[key]) if g != e]
        assert not bad, f"workspace {key[0]}, {key[1]}: {len(bad)} of {len(res)} plans differ from the record, first (problem, got, recorded): {bad[:3]}"
        n += len(res)
    assert n > 6000 and len(got[(1, "table, dense")]) > 900 and len(got[(1, "table, conv stride 1")]) > 400
    # the sections mean what they say: the register-staged ids, a refused forced tile, the in-place strip call on the tiled kernel
    assert all(r != "EINVAL" and r[0] in (9, 10) and r[1] == 1 for r in got[(1, "register-staged")])
    assert "EINVAL" in got[(1, "forced")] and "EINVAL" in got[(1, "GEGLU arguments")]
    assert (12, 1) in got[(1, "forced")] and all(r == "EINVAL" or r[0] > 0 for rs in got.values() for r in rs)
