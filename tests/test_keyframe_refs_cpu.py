"""CPU: the float64 reference of the keyframe kernels (tests/keyframe_refs.py) pinned from both sides -- an f32 emulation of the stated operation order
stays inside the derived bound on every case of the table, four planted defects fall outside it, the reference alone leaves out at most 2 % of a case's
pixels (none on the integer family), its forward-backward criterion is compute_fwdbwd_mask's on the integer family -- and the host side of the key:
hostlogic.keyframe_ids, every refusal of check_keyframes, resolve_generation, the command line and the example configuration."""
import os

import numpy as np
import pytest

import keyframe_refs as R
from tc_light_amd import hostlogic as HL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(R.CASES)


def _excess(got, c):
    """Largest |got - ref| / bound over the pixels that are compared, and the share left out."""
    keep = ~c["left_out"][:, None].repeat(3, axis=1)
    err = np.abs(got.astype(np.float64) - c["out"]) / np.maximum(c["bound"], 1e-300)      # key frames: bound 0, the bits of relit_keys
    return float(err[keep].max()), float(c["left_out"].mean())


@pytest.mark.parametrize("name", NAMES)
def test_f32_emulation_stays_inside_the_bound(name):
    c = R.case(name)
    C32 = R.chain_f32(c["fut"], c["past"], c["keys"])
    out32, holes32, _, _ = R.propagate_ref(c["S"], c["R"], c["keys"], C32, dt=np.float32)
    worst, left_out = _excess(out32, c)
    nonkey = [i for i in range(len(c["S"])) if i not in c["keys"]]
    share = c["left_out"][nonkey].mean() if nonkey else 0.0
    print(f"{name}: f32 emulation max err/bound {worst:.3f}, left out {share:.4f} of the non-key pixels, holes {c['holes'].tolist()}")
    assert worst <= 1.0
    assert share <= R.MAX_AMBIGUOUS
    if R.CASES[name][4] == "integer":
        assert not c["left_out"].any()
        assert np.array_equal(holes32, c["holes"]) and np.array_equal(C32.astype(np.float64), c["C"])
    for k, key in enumerate(c["keys"]):
        assert np.array_equal(c["out"][key], c["R"][k].astype(np.float64))


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n][4] == "smooth"])
def test_smooth_cases_exercise_both_gates_and_holes(name):
    c = R.case(name)
    nonkey = [i for i in range(len(c["S"])) if i not in c["keys"]]
    valid = c["C"][nonkey, :, 2]
    assert 0.0 < valid.mean() < 1.0                               # the forward-backward gate (and the frame's edge) closes somewhere
    assert c["holes"].sum() > 0                                   # the photometric patch: visible in neither key
    assert c["holes"][c["keys"]].sum() == 0


DEFECTS = [("taps clamped where the specification invalidates", dict(chain=dict(clamp_instead_of_invalidate=True))),
           ("ta and tb exchanged", dict(prop=dict(swap_t=True))),
           ("the hole fallback missing", dict(prop=dict(no_hole_fallback=True))),
           ("eps not removed at the end", dict(prop=dict(keep_eps=True)))]


@pytest.mark.parametrize("what,how", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defects_fall_outside_the_bound(what, how):
    caught = []
    for name in NAMES:
        c = R.case(name)
        C = R.chain_ref(c["fut"], c["past"], c["keys"], **how["chain"])[0] if "chain" in how else c["C"]
        out = R.propagate_ref(c["S"], c["R"], c["keys"], C, **how.get("prop", {}))[0]
        if _excess(out, c)[0] > 1.0:
            caught.append(name)
    print(f"{what}: outside the bound on {len(caught)} of {len(NAMES)} cases")
    assert caught, what


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n][4] == "integer"])
def test_forward_backward_criterion_is_the_references_on_integer_flows(name):
    """Bilinear sampling at integer positions is the tap itself, so the squared inequality of the header and compute_fwdbwd_mask's agree exactly."""
    c = R.case(name)
    N, _, H, W = c["fut"].shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for a, b in zip(c["keys"], c["keys"][1:]):
        if b - a < 2:
            continue
        j = a + 1                                                 # distance 1 to the left key: valid = inb && fb
        A = c["past"][j].astype(np.float64)
        qx, qy = xs + A[0], ys + A[1]
        inb = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
        g = R.bil(c["fut"][j - 1].astype(np.float64), qx, qy)
        want = inb & R.fb_of_the_reference(A, g)
        assert np.array_equal(c["C"][j, 0, 2] == 1.0, want)


# ---------------------------------------------------------------------------------------------------------------- the host side
def test_keyframe_ids():
    assert HL.keyframe_ids(9, 4) == [0, 4, 8] and HL.keyframe_ids(6, 4) == [0, 4, 5] and HL.keyframe_ids(2, 16) == [0, 1]
    assert HL.keyframe_ids(5, 2) == [0, 2, 4] and HL.keyframe_ids(17, 16) == [0, 16] and HL.keyframe_ids(1, 4) == [0]
    assert HL.keyframe_ids(3, 7) == [0, 2] and HL.keyframe_ids(300, 4)[-2:] == [296, 299] and len(HL.keyframe_ids(300, 4)) == 76
    assert HL.keyframe_ids(5, 1) == [0, 1, 2, 3, 4]
    for n, k in ((9, 4), (6, 4), (300, 7)):
        assert HL.keyframe_ids(n, k) == R.keyframe_ids(n, k)
        ids = HL.keyframe_ids(n, k)
        assert all(0 < b - a <= k for a, b in zip(ids, ids[1:]))
    with pytest.raises(ValueError):
        HL.keyframe_ids(0, 4)


def test_check_keyframes_normalises():
    full = dict(interval=4, alpha=0.1, diff_threshold=0.1, eps=0.015625)
    assert HL.check_keyframes(None) is None
    assert HL.check_keyframes(4) == full and HL.check_keyframes(dict(interval=4)) == full
    assert HL.check_keyframes(dict(interval=2, alpha=1, eps=0.25)) == dict(interval=2, alpha=1.0, diff_threshold=0.1, eps=0.25)
    assert HL.check_keyframes(1) is None and HL.check_keyframes(dict(interval=1, alpha=0.3)) is None
    # interval 1 is the key switched off: what would be out of scope beside it is not looked at
    assert HL.check_keyframes(1, normal=True, light_path=[[0, 0], [1, 90]], scene_type="sceneflow", post_opt_mode="shard") is None
    assert HL.KEYFRAME_DEFAULTS["eps"] == 1.0 / 64 and HL.KEYFRAME_MAX_INTERVAL == 16


@pytest.mark.parametrize("block,word", [
    (0, "interval"), (17, "interval"), (-1, "interval"), (True, "keyframes"), (2.0, "keyframes"), ("4", "keyframes"), ([4], "keyframes"),
    (dict(interval=2.0), "interval"), (dict(interval=True), "interval"), (dict(alpha=0.1), "keyframes"), (dict(interval=4, every=2), "keyframes"),
    (dict(interval=4, alpha=0), "alpha"), (dict(interval=4, alpha=-1.0), "alpha"), (dict(interval=4, alpha="x"), "alpha"),
    (dict(interval=4, alpha=float("inf")), "alpha"), (dict(interval=4, diff_threshold=0.0), "diff_threshold"),
    (dict(interval=4, diff_threshold=float("nan")), "diff_threshold"), (dict(interval=4, eps=0.0), "eps"), (dict(interval=4, eps=0.26), "eps"),
    (dict(interval=1, eps=0.3), "eps")])
def test_check_keyframes_refuses_by_name(block, word):
    with pytest.raises(ValueError, match=word):
        HL.check_keyframes(block)


@pytest.mark.parametrize("beside,words", [
    (dict(normal=True), ("generation.keyframes", "generation.normal")),
    (dict(light_path=[[0.0, 0.0], [1.0, 90.0]]), ("generation.keyframes", "generation.light_path")),
    (dict(prompt_path=[[0.0, "a"], [1.0, "b"]]), ("generation.keyframes", "generation.prompt_path")),
    (dict(scene_type="sceneflow"), ("generation.keyframes", "data.scene_type")),
    (dict(post_opt_mode="shard"), ("generation.keyframes", "post_opt_mode")),
    (dict(shard_post_opt=True), ("generation.keyframes", "shard_post_opt"))])
def test_check_keyframes_refuses_what_is_out_of_scope_by_both_names(beside, words):
    with pytest.raises(ValueError) as e:
        HL.check_keyframes(4, **beside)
    assert all(w in str(e.value) for w in words)


def test_resolve_generation_and_generator_carry_the_block():
    from types import SimpleNamespace
    import torch
    from tc_light_amd.generate import DEFAULTS, Generator
    assert DEFAULTS["keyframes"] is None and "keyframes" not in HL.RESOLVED_KEYS
    off = HL.resolve_generation(dict(DEFAULTS))
    assert "keyframes" not in off and off == HL.resolve_generation(dict(DEFAULTS, keyframes=1))
    on = HL.resolve_generation(dict(DEFAULTS, keyframes=2))
    assert on["keyframes"] == dict(interval=2, alpha=0.1, diff_threshold=0.1, eps=0.015625)
    assert {k: v for k, v in on.items() if k != "keyframes"} == off
    for bad in (dict(prompt_path=[[0, "a"], [1, "b"]]), dict(scene_type="sceneflow"), dict(post_opt_mode="shard"),
                dict(light_path=[[0, 0], [1, 90]], init_strength=0.5, n_timesteps=2)):
        with pytest.raises(ValueError, match="generation.keyframes"):
            HL.resolve_generation(dict(DEFAULTS, keyframes=2, **bad))
    stub = SimpleNamespace(dev=torch.device("cpu"), tome=SimpleNamespace(args={}))
    assert Generator(stub, None, dict(keyframes=dict(interval=3, eps=0.125), max_tokens_per_pass=1)).cfg.keyframes == dict(
        interval=3, alpha=0.1, diff_threshold=0.1, eps=0.125)
    assert Generator(stub, None, dict(keyframes=1, max_tokens_per_pass=1)).cfg.keyframes is None
    assert Generator(stub, None, dict(max_tokens_per_pass=1)).cfg.keyframes is None
    with pytest.raises(ValueError, match="interval"):
        Generator(stub, None, dict(keyframes=40, max_tokens_per_pass=1))


def test_command_line_and_example_configuration():
    from tc_light_amd.config_utils import DEFAULTS, load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        base = os.path.join("configs", "tclight_default.yaml")
        d = load_config(["--config", base], print_config=False)
        e = load_config(["--config", base, "--keyframes", "4"], print_config=False)
        x = load_config(["--config", os.path.join("configs", "examples", "tclight_keyframes.yaml")], print_config=False)
        y = load_config(["--config", os.path.join("configs", "examples", "tclight_keyframes.yaml"), "--keyframes", "8"], print_config=False)
    finally:
        os.chdir(cwd)
    assert d.generation.keyframes is None and DEFAULTS["generation"]["keyframes"] is None
    assert e.generation.keyframes == 4
    assert HL.check_keyframes(dict(x.generation.keyframes)) == dict(interval=4, alpha=0.1, diff_threshold=0.1, eps=0.015625)
    assert dict(y.generation.keyframes)["interval"] == 8 and x.models.unet


def test_wrapper_tables_and_batches_agree_with_the_reference():
    from tc_light_amd import keyframe
    assert (keyframe.TILE_W, keyframe.TILE_H) == (R.TILE_W, R.TILE_H) and keyframe.MAX_GAP == HL.KEYFRAME_MAX_INTERVAL
    for n, k in ((9, 4), (6, 4), (2, 16), (5, 2), (17, 16), (300, 4), (1, 3)):
        keys = HL.keyframe_ids(n, k)
        h_keys, left, right, tw = keyframe.tables(keys, n)
        l, r, t = R.tables(keys, n)
        assert h_keys.tolist() == keys and left.tolist() == l.tolist() and right.tolist() == r.tolist()
        assert np.array_equal(tw.numpy().view(np.int32), t.view(np.int32))
        b = keyframe.batches(keys)
        assert (b == [] and len(keys) == 1) or ([g0 for g0, _ in b] == [0] + [g1 for _, g1 in b[:-1]] and b[-1][1] == len(keys) - 1)
        assert all(keys[g1] - keys[g0] + 1 <= keyframe.BATCH_FRAMES for g0, g1 in b)
    for bad in ([1, 4], [0, 3], [0, 2, 2, 4], [0, 17, 20]):
        with pytest.raises(ValueError, match="keys"):
            keyframe.tables(bad, bad[-1] + 1 if bad[-1] != 3 else 5)
