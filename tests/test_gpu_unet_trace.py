"""Launch trace of the UNet host path: every C-ABI call of two consecutive `forward_many` passes -- function, every scalar argument, which operands
are null, and the stream it is issued on -- must equal the trace tests/golden/unet_trace.txt recorded (tests/golden/make_golden_unet_trace.py), for the
default route and for every switch of `Switches.from_env` turned the other way.  The host path only sequences launches and owns buffers,
so equal traces + equal FLOP figures + equal bits of the noise prediction say that a restructuring of unet.py / vidtome.py changed nothing.

Inputs: seeded random weights, an 8x12 latent (levels 8x12, 4x6, 2x3, 1x2: levels 0 and 1 merge, level 2 and mid do not), chunks [2, 4, 1, 3] with
injected draws on both coin sides, two passes per variant (the second meets the banks).  One engine serves all variants in a fixed order: the panel
caches, the time embedding and the un-packed text K/V of a variant's first pass are part of what is recorded.

Every non-tensor argument is written as its `repr`, with ONE normalisation: None is written as 0.  Both are the null pointer at the ctypes boundary
(c_void_p), and the host path may pass either for an absent merge map of tcl_gemm_qkv_panels_f16.
"""
import hashlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_trace.txt")
SWITCHES = ["TCL_GN_CONCAT", "TCL_LN_METRIC", "TCL_QKV_PANEL", "TCL_MERGE_LAZY", "TCL_LN_GEMM", "TCL_QPANEL", "TCL_TOME_STREAM", "TCL_CFG_DEDUP"]
VARIANTS = [("default", True, {}), ("cfg_pair=False", False, {})] + [(f"{s}=0", True, {s: "0"}) for s in SWITCHES]
HH, WW, FS, T_STEP = 8, 12, [2, 4, 1, 3], 601.0
DRAWS = [(1, 0.9), (3, 0.2), (-1, 0.7), (0, 0.4)]


class Recorder:
    """Stands in for the ctypes library object: forwards every tcl_* call and appends one line per call to `lines`."""

    def __init__(self, real, main):
        self.real, self.main, self.lines = real, main, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*a):
            args = ["t" if isinstance(x, torch.Tensor) else "0" if x is None else repr(x) for x in a]
            if not name.endswith("_bytes"):                  # every call of the pass but the size queries is a launch: the stream comes last
                args[-1] = "main" if a[-1] == self.main else "side"
            self.lines.append(f"{name}({', '.join(args)})")
            return fn(*a)
        return call


def record_variants():
    """-> ({variant: [trace lines]}, sha256 of the default variant's second noise prediction)."""
    from tc_light_amd import sd15
    from tc_light_amd.unet import UNetEngine
    from tc_light_amd.vidtome import VidToMe
    sd = sd15.random_state_dict(sd15.unet_param_shapes(), seed=1)
    tome = VidToMe("cuda", seed=5)
    eng = UNetEngine(sd, "cuda", tome)
    rec = Recorder(eng.L, torch.cuda.current_stream().cuda_stream)
    eng.L = eng.ops.L = tome.L = rec
    g = torch.Generator(device="cuda").manual_seed(31)
    xh = torch.randn(sum(FS), HH, WW, 8, device="cuda", generator=g).half()
    x = torch.cat([xh, xh]).contiguous()                     # the classifier-free-guidance pair: both halves equal
    text = torch.randn(2, 77, 768, device="cuda", generator=g).half()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    traces, eps_sha = {}, None
    try:
        for name, pair, env in VARIANTS:
            os.environ.update(env)
            tome.reset_global_tokens()
            rec.lines = []
            txt = text.clone()                               # a new text tensor: the variant's first pass packs its K/V, the second finds it packed
            eng.count_flops, eng.flops, eng.flops_executed = True, 0.0, 0.0
            for _ in range(2):
                tome.draws = list(DRAWS)
                eps = eng.forward_many(x, FS, HH, WW, T_STEP, txt, cfg_pair=pair)
                rec.lines += [f"flops={eng.flops!r}", f"flops_executed={eng.flops_executed!r}"]
            torch.cuda.synchronize()
            if name == "default":
                assert torch.isfinite(eps.float()).all()
                eps_sha = hashlib.sha256(eps.cpu().numpy().tobytes()).hexdigest()
            traces[name] = rec.lines
            for k in env:
                del os.environ[k]
    finally:
        tome.reset_global_tokens()
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return traces, eps_sha


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def read_golden():
    """-> ({variant: (line count, sha256)}, eps sha256, [the default variant's lines])."""
    head, _, body = open(GOLDEN).read().partition("--- default\n")
    sums, eps_sha = {}, None
    for ln in head.splitlines():
        if ln.startswith("eps_sha256 "):
            eps_sha = ln.split()[1]
        elif ln and not ln.startswith("#"):
            name, n, sha = ln.rsplit(" ", 2)
            sums[name] = (int(n), sha)
    return sums, eps_sha, body.splitlines()


@pytest.fixture(scope="module")
def recorded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return record_variants()


@pytest.mark.parametrize("variant", [v[0] for v in VARIANTS])
def test_launch_trace_equals_golden(recorded, tmp_path, variant):
    sums, _, default = read_golden()
    got = recorded[0][variant]
    if (len(got), digest(got)) == sums[variant]:
        return
    out = tmp_path / "unet_trace_got.txt"
    out.write_text("\n".join(got) + "\n")
    where = ""
    if variant == "default":
        k = next((i for i, (a, b) in enumerate(zip(got, default)) if a != b), min(len(got), len(default)))
        where = f"; first difference at line {k}: got {got[k] if k < len(got) else '<end>'!r}, golden {default[k] if k < len(default) else '<end>'!r}"
    pytest.fail(f"{variant}: {len(got)} calls (golden {sums[variant][0]}), sha256 differs{where}; the recorded trace is in {out}")


def test_noise_prediction_bits_equal_golden(recorded):
    assert recorded[1] == read_golden()[1]
