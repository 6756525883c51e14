"""GPU: exact per-element leaf parity of tcl_gemm_f16 / tcl_conv3x3_f16 (csrc/gemm.hip, gemm8.hip, gemm8q.hip, linstrip.hip, gemm_conv.h) against
tests/gemm_refs.py (pinned to torch float64 by tests/test_gemm_refs_cpu.py).

Operands lie on a small lattice (integers; multiples of 1/8 for the non-linear epilogues), so every product and every f32 partial sum is exact in any
order and with any K split: a linear epilogue (act 0 / 3) owes the reference's integers BIT FOR BIT on every element, on every tile configuration
that the dispatcher accepts for the case (the case's must_run, asserted against the dispatcher on the CPU: a refused must_run tile and an accepted
tile outside must_run both fail).  No tolerance, no excluded element.

Every output buffer has ldc >= N and four guard rows, prefilled with a sentinel f16 (0x3555, not on any lattice) that must survive outside
[0, M) x [0, N); padding columns of A, W and the residual are NaN, so a kernel that folds one into a sum shows NaN.

Non-linear epilogues (act 1 SiLU, 4 erf-GELU, 5 GELU after the residual, 2 GEGLU): z is exact, the reference is act(z) in float64, and the kernel adds
one f32 evaluation of the activation and one rounding to f16:
    |y - ref| <= ulp_f16(ref) + |z| * 2^-23            (act 2: |value * gate| in place of |z|)
half an f16 ulp for the rounding, the other half as slack for the f32 evaluation; the second term for the absolute error of erf (Abramowitz-Stegun
7.1.26 in gemm_conv.h: < 1.5e-7, times |z| / 2 < |z| 2^-23) where 0.5 z (1 + erf) cancels for negative z.  The tiles must still agree bit for bit.
`-s` prints the figures kept in profiles/gemm_leaf_parity.txt."""
import pytest
import torch
import torch.nn.functional as F

import gemm_refs as R

pytestmark = pytest.mark.gpu
H = torch.float16
SENT = 0x3555                       # f16 0.33325: no multiple of 1/8
GUARD = 4                           # rows behind row M
DENSE = [c for c in R.CASES.values() if c["kind"] == "dense" and c["den"] == 1]
CONV = [c for c in R.CASES.values() if c["kind"] == "conv"]
NONLIN = [c for c in R.CASES.values() if c["den"] != 1]
name = lambda c: c["name"]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def sync():
    """A device error ends the session: nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error in test_gpu_gemm_leaves.py: {e}", returncode=3)


def bits(t):
    return t.contiguous().view(torch.int16)


def sentinel(rows, cols):
    return torch.full((rows, cols), SENT, dtype=torch.int16, device="cuda").view(H)


def padded(t, ld, rows=None):
    """t [r, c] on the device in a [rows, ld] buffer whose other entries are NaN."""
    buf = torch.full((rows or t.shape[0], ld), float("nan"), dtype=H, device="cuda")
    buf[:t.shape[0], :t.shape[1]] = t.cuda()
    return buf


class Problem:
    """One case on the device: operands built once, a fresh guarded output per run."""

    def __init__(self, c):
        self.c, dense = c, c["kind"] == "dense"
        d = self.d = R.make_dense(c) if dense else R.make_conv(c)
        self.ref, self.z, staged = R.reference(c, d)
        self.linear = c["act"] in (0, 3)
        R.assert_exact_ok(self.z, self.ref, c["den"], self.linear, staged)
        W, b = d["W"], d["bias"]
        if c["act"] == 2:
            from tc_light_amd.unet import _geglu_rows
            W, b = _geglu_rows(W), (_geglu_rows(b) if b is not None else None)
        self.bias = b.contiguous().cuda() if b is not None else 0
        if dense:
            self.M, self.No, self.ldc = c["M"], self.ref.shape[1], c["ldc"]
            if c["vae"]:            # A = columns [0, K), W = columns [K, 2K) of one [M, 3K] buffer; the last third stays NaN
                assert c["M"] == c["N"]
                self.buf = padded(torch.cat([d["A"], W], dim=1), 3 * c["K"])
                self.A, self.W = self.buf, self.buf[:, c["K"]:]
            else:
                self.A, self.W = padded(d["A"], c["lda"]), padded(W, c["ldw"])
            self.R = padded(d["resid"], c["ldr"]) if c["resid"] == 1 else None
        else:
            self.M, self.No, self.ldc = self.ref.shape[0] * self.ref.shape[1] * self.ref.shape[2], c["Cout"], c["Cout"]
            self.A, self.W = d["X"].contiguous().cuda(), W.contiguous().cuda()
            self.R = d["resid"].contiguous().cuda() if c["resid"] else None
            self.ref, self.z = self.ref.reshape(self.M, self.No), self.z.reshape(self.M, self.No)
        assert self.ldc >= self.No and self.ref.shape == (self.M, self.No)
        self.want = self.ref.to(H).cuda()

    def run(self, L):
        """-> the whole guarded output buffer [M + GUARD, ldc]; raises RuntimeError when the dispatcher refuses the call."""
        c, out = self.c, sentinel(self.M + GUARD, self.ldc)
        resid = self.R if self.R is not None else 0
        if c["resid"] == 2:
            out[:self.M, :self.No] = self.d["resid"].cuda()
            resid = out
        if c["kind"] == "dense":
            assert self.A.numel() >= (c["M"] - 1) * c["lda"] + c["K"] and out.numel() >= (self.M - 1) * self.ldc + self.No
            L.tcl_gemm_f16(self.A, self.W, self.bias, resid, out, c["M"], c["N"], c["K"], c["lda"], c["ldw"], c["ldc"], c["ldr"], c["act"], st())
        else:
            L.tcl_conv3x3_f16(self.A, self.W, self.bias, resid, out, c["B"], c["Hin"], c["Win"], c["Cin"], c["Cout"], c["stride"], c["pad"], c["Hup"],
                              c["Wup"], c["act"], st())
        sync()
        return out

    def check_guards(self, out, tag):
        o = bits(out).clone()
        o[:self.M, :self.No] = SENT
        bad = (o != SENT).nonzero()
        assert bad.numel() == 0, f"{tag}: {bad.shape[0]} elements outside [0, {self.M}) x [0, {self.No}) written, first at {tuple(bad[0].tolist())}"

    def check_exact(self, out, tag):
        self.check_guards(out, tag)
        got = out[:self.M, :self.No]
        bad = (bits(got) != bits(self.want)).nonzero()
        if bad.numel():
            i, j = bad[0].tolist()
            raise AssertionError(f"{tag}: {bad.shape[0]} of {got.numel()} elements differ from the exact reference, first at ({i}, {j}): "
                                 f"got {got[i, j].item()} want {self.want[i, j].item()}")


def for_each_tile(L, c, body, mn):
    """body(cfg) under every forced tile of the case, then (auto cases) under none; exactly the must_run tiles must have run."""
    ws = None
    ran = []
    try:
        if c["splits"] > 1 or c.get("ws"):
            ws = torch.empty(16 << 20, dtype=torch.uint8, device="cuda")
            assert 8 * mn * 4 <= ws.numel()                 # up to 8 f32 partials of the whole result: the launchers never lower the split
            L.tcl_set_workspace(ws, ws.numel())
        for cfg in c["cfgs"]:
            L.tcl_gemm_tune(cfg, c["splits"])
            try:
                body(cfg)
            except RuntimeError as e:
                assert "TCL_EINVAL" in str(e), f"{c['name']}: cfg {cfg}: {e}"
                continue
            ran.append(cfg)
        assert tuple(ran) == c["must_run"], f"{c['name']}: tiles {tuple(ran)} ran, must_run is {c['must_run']}"
        if c["auto"]:
            L.tcl_gemm_tune(0, 0)
            body(0)
    finally:
        L.tcl_gemm_tune(0, 0)
        L.tcl_set_workspace(0, 0)
        sync()
    return ran


@pytest.mark.parametrize("c", DENSE + CONV, ids=name)
def test_linear_epilogues_are_bit_exact_on_every_tile(L, c):
    """(a) dense and (b) 3x3 convolution cases of gemm_refs.CASES, act 0 / 3."""
    p = Problem(c)
    if c["name"] == "cin320_splitk_auto":       # the automatic choice does split K here once a workspace is registered
        assert c["auto"] and c["ws"] and not c["cfgs"]
    ran = for_each_tile(L, c, lambda cfg: p.check_exact(p.run(L), f"{c['name']} cfg {cfg} splits {c['splits']}"), p.M * p.No)
    print(f"[gemm-leaf] {c['name']}: M {p.M} N {p.No} ldc {p.ldc}: exact on tiles {tuple(ran)}{' and the automatic choice' if c['auto'] else ''}")


@pytest.mark.parametrize("axis", ["H", "W"])
@pytest.mark.parametrize("C,cfg", R.SWEEP_TILES, ids=[f"c{C}_cfg{cfg}" for C, cfg in R.SWEEP_TILES])
def test_nearest_index_sweep(L, C, cfg, axis):
    """(c) identity on the centre tap: Y must be the nearest up-sampling of X bit for bit, at every (n_in, n_up) of the sweep, on one tile of each of
    the three gather implementations."""
    x_all = R.lattice((24 * 4 * C,), tuple(range(-8, 9)), 0.0, 5 + C)
    x_dev = x_all.cuda()
    W = torch.zeros(C, 9 * C, dtype=H)
    W[torch.arange(C), 4 * C + torch.arange(C)] = 1.0
    W = W.cuda()
    n_run = 0
    try:
        L.tcl_gemm_tune(cfg, 1)
        for n_in, n_up in R.SWEEP:
            hin, win, hup, wup = (n_in, 4, n_up, 4) if axis == "H" else (4, n_in, 4, n_up)
            x = x_all[:n_in * 4 * C].view(1, hin, win, C)
            want = F.interpolate(x.float().permute(0, 3, 1, 2), size=(hup, wup), mode="nearest").permute(0, 2, 3, 1).reshape(hup * wup, C).to(H).cuda()
            out = sentinel(hup * wup + GUARD, C)
            try:
                L.tcl_conv3x3_f16(x_dev, W, 0, 0, out, 1, hin, win, C, C, 1, 1, hup, wup, 0, st())
            except RuntimeError as e:
                assert "TCL_EINVAL" in str(e) and not R.sweep_accepts(cfg, n_in, n_up), f"cfg {cfg} refused {axis} {n_in} -> {n_up}: {e}"
                continue
            sync()
            assert R.sweep_accepts(cfg, n_in, n_up)
            n_run += 1
            bad = (bits(out[:hup * wup]) != bits(want)).nonzero()
            assert bad.numel() == 0, (f"cfg {cfg} axis {axis} {n_in} -> {n_up}: {bad.shape[0]} elements differ from F.interpolate, first at output "
                                      f"pixel (y, x) = {divmod(bad[0, 0].item(), wup)}, channel {bad[0, 1].item()}")
            assert bool((bits(out[hup * wup:]) == SENT).all()), f"cfg {cfg} axis {axis} {n_in} -> {n_up}: guard rows written"
    finally:
        L.tcl_gemm_tune(0, 0)
        sync()
    assert n_run == sum(R.sweep_accepts(cfg, i, u) for i, u in R.SWEEP)
    print(f"[gemm-leaf] nearest sweep C {C} cfg {cfg} axis {axis}: {n_run} of {len(R.SWEEP)} ratios ran, all exact")


@pytest.mark.parametrize("c", NONLIN, ids=name)
def test_nonlinear_epilogues_within_one_rounding_of_float64(L, c):
    """(d) per element against act(z) in float64 with the bound of the module docstring; the tiles agree bit for bit."""
    p = Problem(c)
    if c["act"] == 2:
        D = p.No
        slack = (p.z[:, :D] * p.z[:, D:]).abs()
    else:
        slack = p.z.abs()
    bound = R.ulp_f16(p.ref) + slack * 2.0 ** -23
    outs, worst, tight = {}, 0.0, 0.0

    def body(cfg):
        nonlocal worst, tight
        out = p.run(L)
        tag = f"{c['name']} cfg {cfg}"
        p.check_guards(out, tag)
        y = out[:p.M, :p.No].double().cpu()
        assert bool(torch.isfinite(y).all()), f"{tag}: {(~torch.isfinite(y)).sum().item()} non-finite elements, first at {tuple((~torch.isfinite(y)).nonzero()[0].tolist())}"
        err = (y - p.ref).abs()
        worst, tight = max(worst, float((err / R.ulp_f16(p.ref)).max())), max(tight, float((err / bound).max()))
        bad = (err > bound).nonzero()
        if bad.numel():
            i, j = bad[0].tolist()
            raise AssertionError(f"{tag}: {bad.shape[0]} of {y.numel()} elements past the bound, first at ({i}, {j}): got {y[i, j].item()!r} ref "
                                 f"{p.ref[i, j].item()!r} bound {bound[i, j].item():.3e}; largest error {float((err / R.ulp_f16(p.ref)).max()):.3f} f16 ulp")
        outs[cfg] = out[:p.M, :p.No].clone()

    ran = for_each_tile(L, c, body, p.M * c["N"])
    first = outs[ran[0]]
    for cfg, o in outs.items():
        nd = (bits(o) != bits(first)).nonzero()
        assert nd.numel() == 0, f"{c['name']}: cfg {cfg} differs from cfg {ran[0]} in {nd.shape[0]} elements, first at {tuple(nd[0].tolist())}"
    print(f"[gemm-leaf] {c['name']}: act {c['act']} tiles {tuple(ran)}: largest |y - ref| = {worst:.3f} f16 ulp of the reference, "
          f"{tight:.3f} of the bound")
