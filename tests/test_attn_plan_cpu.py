"""The panel sizes and the flash variant of an attention call are decided on the host (csrc/attn_panels.h: attn_panels, csrc/attn.hip: choose).  A size that
drifts makes a producer and the flash kernel disagree about where V^T or the overflow flags start -- valid but wrong memory -- and a re-routed shape is only
a slower benchmark.  The three *_bytes functions and tcl_attention_plan answer without a GPU; this test pins them to tests/golden/attn_plan_gfx950.txt."""
import json
import os
import subprocess
import sys

from tc_light_amd import lib as libmod

EXPECT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plan_gfx950.txt")
DS, BS, HS = (40, 80, 128, 160), (1, 2, 4, 16, 62), (1, 5, 8)
TS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1793, 2048, 8900, 35600)          # on and around every rounding edge of Tqp (256) and Tkp (64)
PACK_KV, PAIR, PREPACKED = libmod.TCL_ATTN_PACK_KV, libmod.TCL_ATTN_PAIR, libmod.TCL_ATTN_PREPACKED
# head_dim 40, (B, H, pair, n = Tqp / 256): B (2 if pair) H n = 1024 selects the two-query-block kernels, whose launch has B H n blocks; the exact pass
# behind the speculative kernel is capped at 512 blocks.  Just below, at and just above both.
EDGES40 = [(1, 1, 0, 1023), (1, 1, 0, 1024), (1, 1, 0, 1025), (1, 1, 1, 511), (1, 1, 1, 512), (1, 1, 1, 513), (16, 8, 0, 7), (16, 8, 0, 8), (16, 8, 0, 9),
           (16, 8, 1, 3), (16, 8, 1, 4), (16, 8, 1, 5), (62, 8, 0, 2), (62, 8, 0, 3), (62, 8, 1, 1), (62, 8, 1, 2), (2, 5, 0, 102), (2, 5, 0, 103),
           (2, 5, 1, 51), (2, 5, 1, 52), (4, 1, 1, 127), (4, 1, 1, 128), (4, 1, 1, 129)]


def sections():
    """[(name, function, [argument tuples])] in the order of the expectation file.  Plan arguments: (B, H, Tq, Tk, d, kv_div, flags)."""
    grid = [(d, B, H, T) for d in DS for B in BS for H in HS for T in TS]
    out = [("q_bytes", "tcl_attention_q_bytes", [(B, H, T, d) for d, B, H, T in grid]),
           ("kv_bytes", "tcl_attention_kv_bytes", [(B, H, T, d) for d, B, H, T in grid]),
           ("splitkv_workspace_bytes", "tcl_attention_splitkv_workspace_bytes",
            [(ns, H, Tq, 64 * ns * m, 128) for ns in (2, 3, 5, 16) for H in HS for Tq in (1, 257, 14400) for m in (1, 7, 150)])]
    sweep = []
    for d in DS:
        for bi, B in enumerate(BS):
            for hi, H in enumerate(HS):
                for i, Tq in enumerate(TS):
                    Tk = TS[(i + bi + hi) % len(TS)]
                    for kv_div in sorted({1, B}):
                        sweep += [(B, H, Tq, Tk, d, kv_div, PACK_KV), (B, H, Tq, Tk, d, kv_div, PACK_KV | PAIR)]
    out.append(("plan, sweep", "plan", sweep))
    out.append(("plan, Tq x Tk", "plan", [(2, 8, Tq, Tk, d, 1, PACK_KV) for d in DS for Tq in TS for Tk in TS]))
    edges = []
    for B, H, pair, n in EDGES40:
        for Tq in (256 * n, 256 * n - 255):                # a full and a ragged last query block
            for p in sorted({pair, 0}):
                edges += [(B, H, Tq, 200, 40, 1, PACK_KV | (PAIR if p else 0)), (B, H, Tq, 4096, 40, B, PREPACKED | (PAIR if p else 0))]
    out.append(("plan, head_dim 40 thresholds", "plan", edges))
    out.append(("plan, refused and flag combinations", "plan", [
        (2, 8, 300, 300, 64, 1, PACK_KV), (0, 8, 300, 300, 40, 1, PACK_KV), (2, 0, 300, 300, 40, 1, PACK_KV), (2, 8, 0, 300, 40, 1, PACK_KV),
        (2, 8, 300, 0, 40, 1, PACK_KV), (2, 8, 300, 300, 40, 0, PACK_KV), (4, 8, 300, 300, 40, 3, PACK_KV), (2, 8, 300, 300, 40, 1, PACK_KV | PREPACKED),
        (16, 8, 2048, 300, 40, 1, PACK_KV | PAIR | PREPACKED), (2, 8, 300, 300, 40, 1, 0), (16, 8, 2048, 300, 40, 1, 0), (16, 8, 1024, 300, 40, 1, PAIR),
        (16, 8, 1024, 300, 40, 1, PREPACKED | PAIR), (2, 8, 300, 300, 80, 2, PREPACKED)]))
    return out


def rows40():
    """The head_dim-40 plan rows: what the TCL_FLASH40 switch can move."""
    return [a for _, fn, rows in sections() if fn == "plan" for a in rows if a[4] == 40]


# A child process for one value of TCL_FLASH40 (the library reads it once per process): loads the library and only asks the plan.
_CHILD = """
import ctypes, json, sys
dll = ctypes.CDLL(sys.argv[1])
out = (ctypes.c_int * 4)()
res = []
for a in json.loads(sys.stdin.read()):
    rc = dll.tcl_attention_plan(*a, out)
    res.append(list(out) if rc == 0 else "EINVAL")
print(json.dumps(res))
"""


def ask_plan(L, args):
    import torch
    out = torch.full((4,), -7, dtype=torch.int32)
    try:
        L.tcl_attention_plan(*args, out)
    except RuntimeError as e:
        assert "TCL_EINVAL" in str(e)
        return "EINVAL"
    return tuple(out.tolist())


def read_expect(path=EXPECT):
    exp, cur = {}, None
    for ln in open(path):
        ln = ln.strip()
        if ln.startswith("== "):
            cur = exp.setdefault(ln[3:], [])
        elif ln and not ln.startswith("#"):
            cur.append("EINVAL" if ln == "EINVAL" else tuple(int(v) for v in ln.split()))
    return exp


def _compare(name, rows, got, exp):
    assert len(got) == len(exp) == len(rows), name
    bad = [(a, g, e) for a, g, e in zip(rows, got, exp) if g != e]
    assert not bad, f"{name}: {len(bad)} of {len(rows)} answers differ from the record, first (arguments, got, recorded): {bad[:3]}"


def test_attention_sizes_and_plan_match_the_record():
    """The expectations were recorded from the code as it was BEFORE AttnPanels and choose() existed: the sizes by calling that build's *_bytes functions,
    the plans from a build whose launch_flash recorded (instance, grid, LDS bytes) instead of launching, asked through tcl_attention_f16 with fake operands.

    One property the record cannot have: a gated second launch BELOW 512 blocks.  The speculative kernel is only chosen when B (2 if pair) H Tqp / 256
    >= 1024, and its launch has B H Tqp / 256 blocks -- at least 512, so the second launch has exactly 512 blocks whether the cap acts (first > 512) or
    not (first == 512).  Both of those cases are asserted instead."""
    L, exp = libmod.lib(), read_expect()
    secs = sections()
    assert [s[0] for s in secs] == [k for k in exp if not k.startswith("TCL_FLASH40")]
    plans = []
    for name, fn, rows in secs:
        got = [ask_plan(L, a) for a in rows] if fn == "plan" else [(getattr(L, fn)(*a),) for a in rows]
        _compare(name, rows, got, exp[name])
        if fn == "plan":
            plans += got
    assert len(plans) > 3900 and "EINVAL" in plans
    ok = [p for p in plans if p != "EINVAL"]
    assert {p[0] for p in ok} == {0, 2, 3, 4, 5}          # every variant of the default mode; 1 (the kill switch's) is in the TCL_FLASH40 = 5 record
    second = [p for p in ok if p[2]]
    assert second and all(p[0] == 0 and p[2] == 512 for p in second)
    assert any(p[1] == 512 for p in second) and any(p[1] > 512 for p in second) and all(p[2] == 0 for p in ok if p[0] != 0)


def test_flash40_switch_in_child_processes():
    """TCL_FLASH40 = 1 (always the one-query-block kernel) and 5 (no speculative softmax) move the head_dim-40 rows as recorded (same probe build, same
    environment); one child after the other."""
    exp, rows = read_expect(), rows40()
    for mode in ("1", "5"):
        env = dict(os.environ, TCL_FLASH40=mode)
        r = subprocess.run([sys.executable, "-c", _CHILD, libmod.LIB_PATH], input=json.dumps(rows), env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [g if g == "EINVAL" else tuple(g) for g in json.loads(r.stdout)]
        _compare(f"TCL_FLASH40={mode}", rows, got, exp[f"TCL_FLASH40={mode}"])
        ids = {g[0] for g in got if g != "EINVAL"}
        assert ids == ({2} if mode == "1" else {1, 2}) and all(g[2] == 0 for g in got if g != "EINVAL")
