"""CPU: what tests/test_gpu_gemm_leaves.py stands on.  (1) gemm_refs.gemm_exact / conv3x3_exact against torch float64 (F.linear, F.conv2d with
F.pad and F.interpolate) on every case of gemm_refs.CASES; nearest_src against F.interpolate on every ratio of the sweep.  (2) the exactness condition
assert_exact_ok on every case, so the GPU test owes no exclusions.  (3) routing, asked of the built library without a GPU (tcl_gemm_plan /
tcl_conv3x3_plan under tcl_gemm_tune): the forced tiles the dispatcher accepts are exactly each case's must_run."""
import shutil

import pytest
import torch
import torch.nn.functional as F

import gemm_refs as R
from tc_light_amd import lib as libmod

CASES = list(R.CASES.values())
ids = [c["name"] for c in CASES]


def torch_ref(c, d):
    """The case in torch float64, by the library routes: F.linear; F.interpolate -> F.pad -> F.conv2d on NCHW."""
    f = lambda t: None if t is None else t.double()
    if c["kind"] == "dense":
        z = F.linear(f(d["A"]), f(d["W"]), f(d["bias"]))
    else:
        x = f(d["X"]).permute(0, 3, 1, 2)
        if c["Hup"]:
            x = F.interpolate(x, size=(c["Hup"], c["Wup"]), mode="nearest")
        if c["pad"] == 0:
            x = F.pad(x, (0, 1, 0, 1))
        w = f(d["W"]).view(c["Cout"], 3, 3, c["Cin"]).permute(0, 3, 1, 2)
        z = F.conv2d(x, w, f(d["bias"]), stride=c["stride"], padding=c["pad"]).permute(0, 2, 3, 1)
    r, act = f(d["resid"]), c["act"]
    if act == 2:
        D = z.shape[-1] // 2
        return z[..., :D] * F.gelu(z[..., D:])
    if act == 5:
        return F.gelu(z + r if r is not None else z)
    y = {0: z, 1: F.silu(z), 3: F.relu(z), 4: F.gelu(z)}[act]
    return y + r if r is not None else y


def data(c):
    return R.make_dense(c) if c["kind"] == "dense" else R.make_conv(c)


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_reference_equals_torch_float64_and_is_exact(c):
    d = data(c)
    out, z, staged = R.reference(c, d)
    ref = torch_ref(c, d)
    assert out.shape == ref.shape
    linear = c["act"] in (0, 3)
    if linear:
        assert torch.equal(out, ref), f"{c['name']}: {(out != ref).sum().item()} elements differ from torch float64"
    else:       # float64 on both sides, another order of the sum and torch's own erf / sigmoid: a few float64 ulps
        assert float((out - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    R.assert_exact_ok(z, out, c["den"], linear, staged)
    # the lattice is not degenerate: at least a quarter of every operand is non-zero, and the results spread
    for k, t in d.items():
        assert t is None or float((t != 0).double().mean()) >= 0.25, k
    assert out.unique().numel() >= (8 if c["act"] != 3 else 4)
    if not linear:      # the activations are exercised where they bend and in both tails
        assert float(z.min()) < -3 and float(z.max()) > 3


def test_geometries_of_the_conv_cases():
    """The table holds what section (b) of the leaf test needs: both strides, both paddings at odd and even sizes, the three kinds of up-sampling,
    planes of height or width 1, batch 1 and 3, every Cin / Cout."""
    cv = [c for c in CASES if c["kind"] == "conv"]
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in cv)
    assert has(stride=1, pad=1, Hin=5, Win=7) and has(Hin=1, Win=1) and has(Hin=1, Win=9) and has(Hin=9, Win=1)
    for stride, pad in ((2, 1), (2, 0)):
        assert has(stride=stride, pad=pad, Hin=7, Win=9) and has(stride=stride, pad=pad, Hin=8, Win=10)
    assert has(Hin=6, Win=5, Hup=11, Wup=9) and has(Hin=5, Win=4, Hup=10, Wup=8) and has(Hin=3, Hup=3, Win=6, Wup=12) and has(Hin=6, Hup=12, Win=3, Wup=3)
    assert {c["Cin"] for c in cv} == {64, 128, 320} and {c["Cout"] for c in cv} >= {64, 128, 192, 320, 640} and {c["B"] for c in cv} == {1, 3}
    dn = [c for c in CASES if c["kind"] == "dense" and c["den"] == 1]
    assert {1, 127, 129, 255, 257, 513, 300} <= {c["M"] for c in dn} and {64, 128, 192, 320, 704} <= {c["K"] for c in dn}
    assert {64, 128, 192, 320, 640, 1280, 4, 77, 100, 516} <= {c["N"] for c in dn}


def test_nearest_src_is_torch_nearest():
    for n_in, n_up in R.SWEEP + [(12, 23), (20, 40), (6, 11), (5, 9), (3, 3)]:
        x = torch.arange(n_in, dtype=torch.float64).view(1, 1, n_in, 1)
        ref = F.interpolate(x, size=(n_up, 1), mode="nearest").view(-1).long()
        assert torch.equal(torch.from_numpy(R.nearest_src(n_in, n_up)), ref), (n_in, n_up)
    assert len(R.SWEEP) == sum(i + 1 for i in range(1, 25))


def test_ulp_f16():
    x = torch.tensor([0.0, 2.0 ** -30, 2.0 ** -14, 1.0, 1.5, 2.0, 2047.0, 2048.0, -3.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 1.0, 2.0, 2.0 ** -9], dtype=torch.float64)
    assert torch.equal(R.ulp_f16(x), want)
    for v in (0.3, 5.7, 100.2, 6.1e-5, 3e-6):      # the spacing torch's own f16 shows
        h = torch.tensor(v).to(R.H)
        nxt = (h.view(torch.int16) + 1).view(R.H)
        assert float(R.ulp_f16(h.double())) == float(nxt.double() - h.double())


# ------------------------------------------------------------------------------------------------------------------------------------------- routing
@pytest.fixture(scope="module")
def L(tmp_path_factory):
    """A private copy of the built library, as in test_gemm_plan_cpu.py: nothing that GPU tests of the same process measured or set reaches it."""
    so = tmp_path_factory.mktemp("gemm_refs") / "libtclight_refs.so"
    shutil.copy(libmod.LIB_PATH, so)
    mp = pytest.MonkeyPatch()
    mp.setattr(libmod, "LIB_PATH", str(so))
    try:
        return libmod._Lib()
    finally:
        mp.undo()


def ask(L, c):
    """-> (cfg, splits), or None where the dispatcher refuses the call."""
    out = torch.full((2,), -7, dtype=torch.int32)
    try:
        (L.tcl_gemm_plan if c["kind"] == "dense" else L.tcl_conv3x3_plan)(*R.plan_args(c), c["resid"], out[0:1], out[1:2])
    except RuntimeError as e:
        assert "TCL_EINVAL" in str(e)
        return None
    return tuple(out.tolist())


def test_must_run_is_what_the_dispatcher_accepts(L):
    try:
        L.tcl_set_workspace(0x7f0000000000, 96 << 20)       # never dereferenced: plans only
        for c in CASES:
            got = {}
            for cfg in R.FORCED:
                L.tcl_gemm_tune(cfg, c["splits"])
                p = ask(L, c)
                if p is not None:
                    got[cfg] = p
            assert tuple(k for k in got if k in c["cfgs"]) == c["must_run"], f"{c['name']}: accepted {tuple(got)}"
            assert all(p[1] == c["splits"] for p in got.values()), c["name"]
            # a forced tile runs as itself -- but for the strip tile on an in-place residual that it would add twice
            reroute = {k: p[0] for k, p in got.items() if p[0] != k}
            assert reroute == ({12: 1} if c["name"] == "inplace_n320_k320" else {}), (c["name"], reroute)
            L.tcl_gemm_tune(0, 0)
            auto = ask(L, c)
            assert auto is not None
            vec = c["N"] % 8 == 0 and c["ldc"] % 8 == 0 and (not c["resid"] or c["ldr"] % 8 == 0) if c["kind"] == "dense" else True
            if not vec:
                assert auto[0] in (9, 10) and auto[1] == 1 and c["must_run"] == (9, 10) and c["auto"], c["name"]
            if c["resid"] == 2:
                assert auto[0] in (1, 3) and c["auto"], f"{c['name']}: in place must take the heuristic tile, not the tuner: {auto}"
            if c["name"] == "cin320_splitk_auto":
                assert auto[1] > 1
        assert sum(c["must_run"] == (9, 10) for c in CASES) >= 8 and sum(12 in c["must_run"] for c in CASES) >= 4
        assert all(any(cfg in c["must_run"] for c in CASES if c["kind"] == kind) for cfg in R.FORCED if cfg != 12 for kind in ("dense", "conv"))
        # the sweep: its tiles accept every ratio they are expected to take, and cfg 15 refuses a scale past 2
        for C, cfg in R.SWEEP_TILES:
            L.tcl_gemm_tune(cfg, 1)
            for n_in, n_up in R.SWEEP:
                for hw in ((n_in, 4, n_up, 4), (4, n_in, 4, n_up)):
                    c = dict(kind="conv", B=1, Hin=hw[0], Win=hw[1], Cin=C, Cout=C, stride=1, pad=1, Hup=hw[2], Wup=hw[3], act=0, resid=0)
                    assert (ask(L, c) is not None) == R.sweep_accepts(cfg, n_in, n_up), (cfg, hw)
    finally:
        L.tcl_gemm_tune(0, 0)
        L.tcl_set_workspace(0, 0)
