"""GPU: leaf parity of the flash attention kernels of csrc/attn.hip -- every row of g_flash, the gated exact pass behind the speculative d = 40 kernel,
split-KV -- each through the C ABI against a float64 evaluation of the same attention on the kernel's own rounded inputs (tests/attn_refs.py; the bound is
pinned on the CPU, from both sides, by tests/test_attn_refs_cpu.py).

Every call: the output is padded (ldo = H d + 8, three rows behind each sample) and prefilled with the f16 sentinel, workspaces are prefilled with 0xFF bytes,
Q / K / V are column slices of fused tensors (ld = 3 H d; K | V at ld = 2 H d for the kv_div cases; ldq = 256 for head_dim 128) whose unused rows hold the
sentinel, and everything is compared on the host in float64.  Samples beyond four: the reference covers the first, the last and every spiked sample; the
NaN and sentinel checks cover all of them.

Classes of assertion
  elementwise  |got - ref| <= 2^-10 |ref| + cA A + Tk 2^-22 max|v| + atol (attn_refs.py), no NaN, every element outside [b, :Tq, :H d] still the sentinel,
               the plan id of tcl_attention_plan equal to the variant the table names.  Largest fraction of the bound per variant in the recorded run
               (profiles/attn_leaf_parity.txt): d40 speculative 0.489, d40 qb2 exact 0.324 (gated pass and TCL_FLASH40 = 5), d40 qb1 0.506 (Tk = 2),
               d80 0.322, d128 0.356, d160 0.382, split-KV 0.330.  The CPU emulation of the same arithmetic reaches 0.506 on the same case.
  exact        torch.equal on bits: a second call on the packed K / V, tcl_attention_pack_f16 + PREPACKED, a dense output against the padded one's valid
               region, kv_div = 2 against K / V repeated, tcl_attention_kvindex_f16 against both, a permuted table against K / V gathered on the host.
  flags        the overflow flags behind the Q panel: set for exactly the spiked blocks (gain 3.2), for none (gain 1.6).
Not entered: the `base += 256` window step of the gated pass in k_flash (it needs more than 131 072 query blocks, a multi-GB Q panel) -- the one line of
k_flash these tests leave out.  Every check prints its figures (`-s`)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import attn_refs as R

pytestmark = pytest.mark.gpu
PACK_KV, PREPACKED = 1, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST, _REACHED = {}, set()          # this run's largest fraction of the bound per variant, and the variants a check ran on


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tc_light_amd.lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int16)


def ff_bytes(n):
    return torch.full((int(n),), 0xFF, dtype=torch.uint8, device="cuda")


def plan_of(L, c, flags=PACK_KV):
    out = torch.full((4,), -7, dtype=torch.int32)
    L.tcl_attention_plan(c.B, c.H, c.Tq, c.Tk, c.d, c.kv_div, flags, out)
    return out.tolist()


class Operands:
    """Device operands of a case in its layout (attn_refs.Case.layout).  q / k / v: the pointers' tensors (views into the fused ones), ld*, *bs in halves."""

    def __init__(self, c, q, k, v):
        C, B, Bkv = c.H * c.d, q.shape[0], k.shape[0]
        if c.layout == "qkv":
            T = max(c.Tq, c.Tk)
            f = R.sentinel16(B, T, 3 * C)
            f[:, :c.Tq, :C], f[:, :c.Tk, C:2 * C], f[:, :c.Tk, 2 * C:] = q, k, v
            self.fused = f.cuda()
            self.q, self.k, self.v = self.fused, self.fused[0, 0, C:], self.fused[0, 0, 2 * C:]
            self.ldq = self.ldk = self.ldv = 3 * C
            self.qbs = self.kbs = self.vbs = T * 3 * C
        else:                                   # "kv": Q dense; "ld256": Q the first C columns of a 2C-wide tensor.  K | V fused at ld = 2C in both
            wq = C if c.layout == "kv" else 2 * C
            fq, fkv = R.sentinel16(B, c.Tq, wq), R.sentinel16(Bkv, c.Tk, 2 * C)
            fq[:, :, :C], fkv[:, :, :C], fkv[:, :, C:] = q, k, v
            self.fq, self.fkv = fq.cuda(), fkv.cuda()
            self.q, self.k, self.v = self.fq, self.fkv, self.fkv[0, 0, C:]
            self.ldq, self.qbs, self.ldk, self.kbs = wq, c.Tq * wq, 2 * C, c.Tk * 2 * C
            self.ldv, self.vbs = self.ldk, self.kbs

    def qkv(self):
        return (self.q, self.ldq, self.qbs, self.k, self.ldk, self.kbs, self.v, self.ldv, self.vbs)


def padded_out(c, B=None):
    """-> (o [B, Tq + 3, H d + 8] sentinel-filled, ldo, obs)."""
    ldo = c.H * c.d + 8
    return R.sentinel16(B or c.B, c.Tq + 3, ldo).cuda(), ldo, (c.Tq + 3) * ldo


def workspaces(L, c, Bkv=None):
    return ff_bytes(L.tcl_attention_q_bytes(c.B, c.H, c.Tq, c.d)), ff_bytes(L.tcl_attention_kv_bytes(Bkv or c.B // c.kv_div, c.H, c.Tk, c.d))


def attention(L, c, ops, o, ldo, obs, flags, wq, wkv, kv_div=None):
    L.tcl_attention_f16(*ops.qkv(), o, ldo, obs, c.B, c.H, c.Tq, c.Tk, c.d, R.f32_scale(c.d), c.kv_div if kv_div is None else kv_div, flags, wq, wkv, st())


def valid_and_clean(c, o):
    """o [B, Tq + 3, ldo] from the device -> its valid region [B, Tq, H d] on the host, after asserting that everything else is still the sentinel."""
    oc = o.cpu()
    C = c.H * c.d
    got = oc[:, :c.Tq, :C].clone()
    oc.view(torch.int16)[:, :c.Tq, :C] = R.SENT16
    assert R.is_sentinel16(oc), "an element outside [b, :Tq, :H d] was written"
    return got


def check_bound(c, kind, got, r, tag, variant):
    """got [n, Tq, H d] f16 on the host, the samples of r: the elementwise bound, and the spiked rows on their own."""
    got = R.heads(got, c)
    frac, row, rel = R.figures(got, r.ref, r.bound)
    print(f"[attn] {tag} {R.case_id(c)} {kind}: worst elementwise fraction {frac:.3f} of the bound (atol {r.atol:.2e}), worst-row rel-L2 {row:.2e}, rel-L2 {rel:.2e}")
    assert frac <= 1.0, (R.case_id(c), kind, frac, row, rel)
    for b, qrow, key in R.spikes(c, kind):
        i = r.samples.index(b)
        fs, rs, _ = R.figures(got[i, qrow], r.ref[i, qrow], r.bound[i, qrow])
        print(f"[attn]     spiked row (sample {b}, query {qrow}, key {key}): fraction {fs:.3f}, worst head rel-L2 {rs:.2e}")
        assert fs <= 1.0, (R.case_id(c), kind, b, qrow, fs)
    _WORST[variant] = max(_WORST.get(variant, 0.0), frac)
    _REACHED.add(variant)


def full_inputs(c, kind, gain=None):
    """Inputs of all B samples (attn_refs.sample_x keeps the draws of the last case, so the kinds of one case share them)."""
    return R.inputs(c, kind, None, gain)


# ================================================================================================================== 1: elementwise, the whole table
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_flash_elementwise(L, c, kind):
    assert plan_of(L, c)[0] == c.variant, "the shape is routed to another kernel than the table says"
    q, k, v, _ = full_inputs(c, kind)
    ops = Operands(c, q, k, v)
    o, ldo, obs = padded_out(c)
    wq, wkv = workspaces(L, c)
    attention(L, c, ops, o, ldo, obs, PACK_KV, wq, wkv)
    torch.cuda.synchronize()
    got = valid_and_clean(c, o)
    assert not torch.isnan(got.float()).any()
    r = R.reference(c, kind)
    check_bound(c, kind, got[list(r.samples)], r, "flash", c.variant)
    if kind == "v_ones":
        assert (got.float() - 1).abs().max().item() <= 2.0 ** -10          # all samples: within one rounding of 1


@pytest.mark.parametrize("kind", R.SPLIT_KINDS)
@pytest.mark.parametrize("c", R.SPLIT_CASES, ids=R.case_id)
def test_splitkv_elementwise(L, c, kind):
    q, k, v, _ = full_inputs(c, kind)
    ops = Operands(c, q, k, v)
    o, ldo, _ = padded_out(c)
    ws = ff_bytes(L.tcl_attention_splitkv_workspace_bytes(c.nsplit, c.H, c.Tq, c.Tk, c.d))
    L.tcl_attention_splitkv_f16(ops.q, ops.ldq, ops.k, ops.ldk, ops.v, ops.ldv, o, ldo, c.H, c.Tq, c.Tk, c.d, R.f32_scale(c.d), c.nsplit, ws, st())
    torch.cuda.synchronize()
    got = valid_and_clean(c, o)
    assert not torch.isnan(got.float()).any()
    check_bound(c, kind, got, R.reference(c, kind), "split-KV", R.SPLITKV)


# ================================================================================================================== 2: exact classes
def _table_case(variant, Tq, Tk):
    return next(c for c in R.CASES if (c.variant, c.Tq, c.Tk) == (variant, Tq, Tk))


EXACT_CASES = (_table_case(R.FV_40_QB1, 300, 321), _table_case(R.FV_40_SPEC, 130, 129), _table_case(R.FV_80, 260, 154), _table_case(R.FV_80, 129, 77),
               _table_case(R.FV_160, 129, 193), _table_case(R.FV_128, 300, 192))


@pytest.mark.parametrize("c", EXACT_CASES, ids=R.case_id)
def test_repacked_prepacked_and_dense_output_same_bits(L, c):
    q, k, v, _ = full_inputs(c, "noise")
    ops = Operands(c, q, k, v)
    wq, wkv = workspaces(L, c)
    o1, ldo, obs = padded_out(c)
    attention(L, c, ops, o1, ldo, obs, PACK_KV, wq, wkv)
    o2 = padded_out(c)[0]
    attention(L, c, ops, o2, ldo, obs, 0, wq, wkv)                               # Q packed again, K / V panels as they are
    assert torch.equal(bits(o2), bits(o1)), "second call with pack_kv = 0 on the same workspaces"
    wq3, wkv3 = workspaces(L, c)
    L.tcl_attention_pack_f16(*ops.qkv(), c.B, c.H, c.Tq, c.Tk, c.d, R.f32_scale(c.d), c.kv_div, PACK_KV, wq3, wkv3, st())
    o3 = padded_out(c)[0]
    attention(L, c, ops, o3, ldo, obs, PREPACKED, wq3, wkv3)
    assert torch.equal(bits(o3), bits(o1)), "tcl_attention_pack_f16 + PREPACKED"
    C = c.H * c.d
    o4 = R.sentinel16(c.B, c.Tq, C).cuda()
    attention(L, c, ops, o4, C, c.Tq * C, PACK_KV, wq, wkv)
    assert torch.equal(bits(o4), bits(o1[:, :c.Tq, :C])), "dense output (ldo = H d)"
    assert not torch.isnan(o4.float()).any()


KV_SHARED = (R._case(R.FV_40_SPEC, 40, 128, 8, 130, 77, kv_div=2), _table_case(R.FV_80, 129, 77), R._case(R.FV_160, 160, 4, 8, 129, 77, kv_div=2))


@pytest.mark.parametrize("c", KV_SHARED, ids=R.case_id)
def test_shared_and_indexed_kv_same_bits(L, c):
    """kv_div = 2 == K / V repeated with kv_div = 1 == the index table b // 2; a permuted table == K / V gathered on the host."""
    assert plan_of(L, c)[0] == c.variant and c.layout == "kv"
    q, k, v, _ = full_inputs(c, "noise")
    ops = Operands(c, q, k, v)
    Bkv = c.B // c.kv_div
    o1, ldo, obs = padded_out(c)
    attention(L, c, ops, o1, ldo, obs, PACK_KV, *workspaces(L, c))

    def gathered(table):
        og = padded_out(c)[0]
        attention(L, c, Operands(c, q, k[table], v[table]), og, ldo, obs, PACK_KV, *workspaces(L, c, c.B), kv_div=1)
        return og

    def indexed(table):
        oi = padded_out(c)[0]
        host = table.to(torch.int32)
        dtab = host.cuda()
        L.tcl_attention_kvindex_f16(*ops.qkv(), oi, ldo, obs, c.B, c.H, c.Tq, c.Tk, c.d, R.f32_scale(c.d), 1, PACK_KV, *workspaces(L, c), dtab, host, Bkv, st())
        torch.cuda.synchronize()
        return oi

    div = R.kv_map(c)
    perm = (7 * torch.arange(c.B) + 3) % Bkv
    assert sorted(set(perm.tolist())) == list(range(Bkv)) and not torch.equal(perm, div)
    assert torch.equal(bits(gathered(div)), bits(o1)), "kv_div = 2 against K / V repeated"
    assert torch.equal(bits(indexed(div)), bits(o1)), "index table b // kv_div against kv_div"
    assert torch.equal(bits(indexed(perm)), bits(gathered(perm))), "permuted index table against K / V gathered on the host"
    got = valid_and_clean(c, o1)
    assert not torch.isnan(got.float()).any()


# ================================================================================================================== 3: the gated exact pass at leaf size
@pytest.mark.parametrize("gain,flagged", [(R.GUARD_GAIN, False), (R.OVERFLOW_GAIN, True)])
def test_gated_exact_pass_small(L, gain, flagged):
    """B = 128, H = 8, Tq = 130, Tk = 256: 1024 blocks of the speculative kernel, 512 of the gated pass (two items each).  attn_refs.overflow_spikes:
    three (sample, query, key, head) with the key gain x q.  Gain 3.2 overflows P inside tile 1 / tile 3: exactly those blocks are flagged, two of them
    items of ONE gated block, and the exact kernel's redo meets the bound on every row.  Gain 1.6 (guard + rebase, no overflow) sets no flag."""
    c = R.GATED
    assert plan_of(L, c)[:3] == [R.FV_40_SPEC, 1024, 512]
    q, k, v, _ = full_inputs(c, "overflow", gain)
    ops = Operands(c, q, k, v)
    o, ldo, obs = padded_out(c)
    wq, wkv = workspaces(L, c)
    attention(L, c, ops, o, ldo, obs, PACK_KV, wq, wkv)
    torch.cuda.synchronize()
    Tqp = -(-c.Tq // 256) * 256
    nblk, panel = c.B * c.H * (Tqp // 256), c.B * c.H * Tqp * 48 * 2                         # Q panel rows of DP = 48 halves (csrc/attn_panels.h)
    off = -(-panel // 256) * 256
    assert int(L.tcl_attention_q_bytes(c.B, c.H, c.Tq, c.d)) == panel + 256 + c.B * c.H * (Tqp // 128) * 4 and off + 8 * nblk <= wq.numel()
    words = wq[off:off + 8 * nblk].view(torch.int32).cpu()                                   # one int per 128-query block is reserved, one per 256 is used
    flags = words[:nblk]
    want = sorted(b * c.H + h for b, _, _, h in R.overflow_spikes(c)) if flagged else []
    print(f"[attn] gated pass, gain {gain}: flagged blocks {flags.nonzero().flatten().tolist()} (expected {want})")
    assert set(flags.unique().tolist()) <= {0, 1} and flags.nonzero().flatten().tolist() == want
    assert (words[nblk:] == -1).all(), "flag words behind the launch's blocks were written"
    got = valid_and_clean(c, o)
    assert not torch.isnan(got.float()).any()
    r = R.reference(c, "overflow", gain)
    check_bound(c, f"overflow x{gain}", got[list(r.samples)], r, "gated" if flagged else "guard", R.FV_40_QB2 if flagged else R.FV_40_SPEC)
    gh = R.heads(got, c)
    for b, row, key, h in R.overflow_spikes(c):                  # the spiked (row, head) itself: about v[key]
        i = r.samples.index(b)
        fs = R.figures(gh[b, row, h], r.ref[i, row, h], r.bound[i, row, h])[0]
        print(f"[attn]     spiked (sample {b}, query {row}, head {h}, key {key}): fraction {fs:.3f}")
        assert fs <= 1.0


# ================================================================================================================== 4: the TCL_FLASH40 kill switches
# One child process per value (the library reads the switch once per process).  Stands on torch and tc_light_amd.lib alone: the inputs are the `noise`
# recipe of attn_refs.sample_x restated.  argv: repository root, job file (json), result file (torch.save).
_CHILD = """
import json, sys, torch
sys.path.insert(0, sys.argv[1])
from tc_light_amd.lib import lib
job, L, res = json.load(open(sys.argv[2])), lib(), {}
st = torch.cuda.current_stream().cuda_stream
for name, B, H, Tq, Tk, d, seed, keep in job["cases"]:
    plan = torch.zeros(4, dtype=torch.int32)
    L.tcl_attention_plan(B, H, Tq, Tk, d, 1, 1, plan)
    assert plan[0].item() == job["variant"], (name, plan.tolist())
    C, T, ldo = H * d, max(Tq, Tk), H * d + 8
    x = torch.stack([torch.randn(T, 3 * C, generator=torch.Generator().manual_seed(seed * 4096 + b)).half() for b in range(B)]).cuda()
    o = torch.full((B, Tq + 3, ldo), job["sentinel"], dtype=torch.int16, device="cuda").view(torch.float16)
    wq = torch.full((L.tcl_attention_q_bytes(B, H, Tq, d),), 255, dtype=torch.uint8, device="cuda")
    wkv = torch.full((L.tcl_attention_kv_bytes(B, H, Tk, d),), 255, dtype=torch.uint8, device="cuda")
    L.tcl_attention_f16(x, 3 * C, T * 3 * C, x[0, 0, C:], 3 * C, T * 3 * C, x[0, 0, 2 * C:], 3 * C, T * 3 * C, o, ldo, (Tq + 3) * ldo, B, H, Tq, Tk, d,
                        torch.tensor(d ** -0.5, dtype=torch.float32).item(), 1, 1, wq, wkv, st)
    torch.cuda.synchronize()
    oc = o.cpu()
    kept = oc[keep].clone()
    nan = bool(torch.isnan(oc[:, :Tq, :C].float()).any())
    oi = oc.view(torch.int16)
    oi[:, :Tq, :C] = job["sentinel"]
    res[name] = {"o": kept, "nan": nan, "clean": bool((oi == job["sentinel"]).all())}
torch.save(res, sys.argv[3])
"""


def test_flash40_kill_switches_in_child_processes(L, tmp_path):
    """TCL_FLASH40 = 1 (the one-query-block kernel) and 5 (the exact two-query-block kernel, no speculative softmax) on the speculative rows of the table:
    the plan id moves to 2, then 1, and the outputs meet the same bound.  A child that fails or times out fails the test; nothing is started after it."""
    cases = [c for c in R.CASES if c.variant == R.FV_40_SPEC]
    for mode, variant in (("1", R.FV_40_QB1), ("5", R.FV_40_QB2)):
        job, out = tmp_path / f"job{mode}.json", tmp_path / f"out{mode}.pt"
        job.write_text(json.dumps({"variant": variant, "sentinel": R.SENT16,
                                   "cases": [[R.case_id(c), c.B, c.H, c.Tq, c.Tk, c.d, c.seed, list(R.subset(c))] for c in cases]}))
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(job), str(out)], env=dict(os.environ, TCL_FLASH40=mode), capture_output=True, text=True,
                           timeout=240)
        assert p.returncode == 0, (mode, p.stdout[-1000:], p.stderr[-3000:])
        res = torch.load(out)
        for c in cases:
            e = res[R.case_id(c)]
            assert e["clean"] and not e["nan"], (mode, R.case_id(c))
            r = R.reference(c, "noise")
            check_bound(c, "noise", e["o"][:, :c.Tq, :c.H * c.d], r, f"TCL_FLASH40={mode}", variant)


# ================================================================================================================== 5: refused arguments
def test_refused_arguments(L):
    """TCL_EINVAL before any launch: the sentinel-filled output stays as it was."""
    c = R._case(R.FV_40_QB1, 40, 4, 8, 129, 65)
    q, k, v, _ = full_inputs(c, "noise")
    ops = Operands(c, q, k, v)
    o, ldo, obs = padded_out(c)
    wq, wkv = ff_bytes(2 * L.tcl_attention_q_bytes(c.B, c.H, c.Tq, 48)), ff_bytes(2 * L.tcl_attention_kv_bytes(c.B, c.H, c.Tk, 48))
    sc = R.f32_scale(c.d)
    null_k = (ops.q, ops.ldq, ops.qbs, 0, ops.ldk, ops.kbs, ops.v, ops.ldv, ops.vbs)
    refused = {
        "d = 48": lambda: L.tcl_attention_f16(*ops.qkv(), o, ldo, obs, c.B, c.H, c.Tq, c.Tk, 48, sc, 1, PACK_KV, wq, wkv, st()),
        "B % kv_div": lambda: L.tcl_attention_f16(*ops.qkv(), o, ldo, obs, c.B, c.H, c.Tq, c.Tk, c.d, sc, 3, PACK_KV, wq, wkv, st()),
        "PACK_KV | PREPACKED": lambda: L.tcl_attention_f16(*ops.qkv(), o, ldo, obs, c.B, c.H, c.Tq, c.Tk, c.d, sc, 1, PACK_KV | PREPACKED, wq, wkv, st()),
        "PACK_KV, null K": lambda: L.tcl_attention_f16(*null_k, o, ldo, obs, c.B, c.H, c.Tq, c.Tk, c.d, sc, 1, PACK_KV, wq, wkv, st()),
    }
    s = R._case(R.SPLITKV, 128, 1, 1, 129, 1088, nsplit=17)
    sq, sk, sv, _ = full_inputs(s, "noise")
    sops = Operands(s, sq, sk, sv)
    so, sldo, _ = padded_out(s)
    ws = ff_bytes(max(L.tcl_attention_splitkv_workspace_bytes(16, s.H, s.Tq, 2048, s.d), L.tcl_attention_splitkv_workspace_bytes(2, s.H, s.Tq, 1024, s.d)))
    split = lambda Tk, ns, ld: L.tcl_attention_splitkv_f16(sops.q, sops.ldq, sops.k, sops.ldk, sops.v, sops.ldv, so, ld, s.H, s.Tq, Tk, s.d,   # noqa: E731
                                                           R.f32_scale(s.d), ns, ws, st())
    refused.update({"split-KV, Tk % (64 nsplit)": lambda: split(192, 2, sldo), "split-KV, nsplit = 1": lambda: split(1024, 1, sldo),
                    "split-KV, nsplit = 17": lambda: split(1088, 17, sldo), "split-KV, ldo < H d": lambda: split(1024, 2, 120)})
    for name, call in refused.items():
        with pytest.raises(RuntimeError, match="TCL_EINVAL"):
            call()
        torch.cuda.synchronize()
        assert R.is_sentinel16(o.cpu()) and R.is_sentinel16(so.cpu()), name
        print(f"[attn] refused: {name}")
    assert bool((wq == 0xFF).all()) and bool((wkv == 0xFF).all()) and bool((ws == 0xFF).all())
    split(1024, 2, sldo)                                                           # the same operands are accepted once the arguments are valid
    torch.cuda.synchronize()
    assert not torch.isnan(valid_and_clean(s._replace(Tk=1024, nsplit=2), so).float()).any()


# ================================================================================================================== the run's figures
def test_every_variant_reached_and_worst_fractions():
    """Prints the largest fraction of the bound per variant (what the module docstring quotes).  When the whole file ran: all six rows of g_flash and split-KV
    were reached -- d40 qb2 exact through the gated pass and through TCL_FLASH40 = 5."""
    for vid in sorted(_WORST):
        print(f"[attn] worst elementwise fraction, {(R.FV_NAMES + ('split-KV',))[vid]}: {_WORST[vid]:.3f}")
    if len(_REACHED) > 1:
        assert _REACHED == set(range(7)), _REACHED
