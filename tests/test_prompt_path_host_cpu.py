"""CPU: the host side of generation.prompt_path (hostlogic.check_prompt_path / prompt_table / prompt_sweep, --prompt_sweep, run.py's refusals) and the
float sequence of tcl_text_lerp_f16 as tests/prompt_refs.py restates it."""
import os

import numpy as np
import pytest

import prompt_refs as PR
from tc_light_amd import hostlogic as HL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, C = "sunrise, soft pink light", "noon, white daylight", "dusk, warm orange light"


# ---------------------------------------------------------------------------------------------------------------- check_prompt_path
def test_check_prompt_path_accepts():
    assert HL.check_prompt_path(None) is None
    assert HL.check_prompt_path(None, normal=True, highres_scale=2.0) is None            # off: nothing else is looked at
    assert HL.check_prompt_path([[0, A]]) == [[0.0, A]]                                  # a single keyframe: a constant path
    assert HL.check_prompt_path([[0, A], [1, B]]) == [[0.0, A], [1.0, B]]
    assert HL.check_prompt_path(((0, A), (0.25, B), (1.0, C))) == [[0.0, A], [0.25, B], [1.0, C]]
    assert HL.check_prompt_path([[0, A], [1, A]], normal=False, highres_scale=1) == [[0.0, A], [1.0, A]]


@pytest.mark.parametrize("bad", [
    [], "sunrise", 3, {"0": A},                                   # not a list of keyframes
    [[0, A, 1]], [[0]], [A], [0, A],                              # a keyframe that is not [pos, prompt]
    [["0", A]], [[True, A]], [[float("nan"), A]], [[float("inf"), A]],       # pos not a finite number
    [[0, 7]], [[0, None]], [[0, ""]], [[0, "  "]], [[0, [A]]],   # prompt not a non-empty string
    [[0.1, A], [1, B]], [[1, A]],                                 # the first keyframe is not at 0
    [[0, A], [0.9, B]],                                           # the last is not at 1
    [[0, A], [0.5, B], [0.5, C], [1, A]],                         # not STRICTLY increasing
    [[0, A], [0.7, B], [0.3, C], [1, A]],
    [[0, A], [1, B], [1, C]],
    [[-0.5, A], [0, B], [1, C]],
])
def test_check_prompt_path_refuses_malformed(bad):
    with pytest.raises(ValueError, match=r"generation\.prompt_path"):
        HL.check_prompt_path(bad)


def test_check_prompt_path_refuses_combinations_by_both_names():
    with pytest.raises(ValueError) as e:
        HL.check_prompt_path([[0, A], [1, B]], normal=True)
    assert "generation.prompt_path" in str(e.value) and "generation.normal" in str(e.value)
    for scale in (1.5, 2, 3.0):
        with pytest.raises(ValueError) as e:
            HL.check_prompt_path([[0, A], [1, B]], highres_scale=scale)
        assert "generation.prompt_path" in str(e.value) and "generation.highres_scale" in str(e.value)
    # a malformed list is reported as such, whatever it is combined with
    with pytest.raises(ValueError, match="keyframe"):
        HL.check_prompt_path([[0, 5]], normal=True)


def test_generator_defaults_leave_the_key_off():
    from tc_light_amd.generate import DEFAULTS
    assert DEFAULTS["prompt_path"] is None


# ---------------------------------------------------------------------------------------------------------------- the frame -> (k0, k1, t) table
def test_prompt_table_one_frame_takes_the_first_key():
    assert HL.prompt_table([[0.0, A], [1.0, B]], 1) == ([A, B], [(0, 0, 0.0)], [0])
    assert HL.prompt_table([[0.0, A]], 1) == ([A], [(0, 0, 0.0)], [0])


def test_prompt_table_two_frames_sit_on_the_keyframes():
    prompts, rows, index = HL.prompt_table([[0.0, A], [1.0, B]], 2)
    assert prompts == [A, B] and rows == [(0, 0, 0.0), (1, 1, 0.0)] and index == [0, 1]


def test_prompt_table_five_frames():
    prompts, rows, index = HL.prompt_table([[0.0, A], [1.0, B]], 5)
    assert prompts == [A, B] and index == [0, 1, 2, 3, 4]
    assert rows == [(0, 0, 0.0), (0, 1, 0.25), (0, 1, 0.5), (0, 1, 0.75), (1, 1, 0.0)]
    # three keyframes, the middle one on frame 2: frames on a keyframe copy it (t = 0), the others blend their own segment in f64
    prompts, rows, index = HL.prompt_table([[0.0, A], [0.5, B], [1.0, C]], 5)
    assert prompts == [A, B, C] and index == [0, 1, 2, 3, 4]
    assert rows == [(0, 0, 0.0), (0, 1, 0.5), (1, 1, 0.0), (1, 2, 0.5), (2, 2, 0.0)]
    # a keyframe between two frames: t = (pos - p0)/(p1 - p0) as Python computes it
    _, rows, _ = HL.prompt_table([[0.0, A], [0.3, B], [1.0, C]], 5)
    assert rows == [(0, 0, 0.0), (0, 1, 0.25 / 0.3), (1, 2, (0.5 - 0.3) / (1.0 - 0.3)), (1, 2, (0.75 - 0.3) / (1.0 - 0.3)), (2, 2, 0.0)]
    for _, _, t in rows:
        assert 0.0 <= t < 1.0


def test_prompt_table_deduplicates_rows_and_prompts():
    # a constant path: one row for every frame, whatever N
    assert HL.prompt_table([[0.0, A]], 5) == ([A], [(0, 0, 0.0)], [0] * 5)
    # a sweep between two equal prompts is a constant path too: one prompt to encode, one row, and that row is the prompt's own bits (t = 0)
    assert HL.prompt_table([[0.0, A], [1.0, A]], 5) == ([A], [(0, 0, 0.0)], [0] * 5)
    # A -> B -> A: the prompt is encoded once, the first and the last frame share a row; a held segment (B, B) is one row
    prompts, rows, index = HL.prompt_table([[0.0, A], [0.25, B], [0.75, B], [1.0, A]], 5)
    assert prompts == [A, B] and rows == [(0, 0, 0.0), (1, 1, 0.0)] and index == [0, 1, 1, 1, 0]
    prompts, rows, index = HL.prompt_table([[0.0, A], [0.5, B], [1.0, A]], 9)
    assert prompts == [A, B] and len(rows) == 8 and index == [0, 1, 2, 3, 4, 5, 6, 7, 0]      # the last frame is A again; (0, 1, t) and (1, 0, t) differ
    assert rows[1] == (0, 1, 0.25) and rows[5] == (1, 0, 0.25)


def test_prompt_sweep_expansion_and_cli(tmp_path):
    assert HL.prompt_sweep(A, B) == [[0.0, A], [1.0, B]]
    assert HL.check_prompt_path(HL.prompt_sweep(A, B)) == [[0.0, A], [1.0, B]]
    from tc_light_amd.config_utils import load_config
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation: {{prompt: {{edit: "warm light"}}}}
""")
    c = load_config(["--config", str(cfg), "--prompt_sweep", A, B], print_config=False)
    assert c.generation.prompt_path == HL.prompt_sweep(A, B) and dict(c.generation.prompt) == {"edit": "warm light"}
    c = load_config(["--config", str(cfg)], print_config=False)
    assert c.generation.get("prompt_path") is None


def test_prompt_table_rank_slicing_at_world_two():
    path = [[0.0, A], [0.5, B], [1.0, C]]
    n = 5
    prompts, rows, index = HL.prompt_table(path, n)
    seen = []
    for rank in range(2):
        lo, hi = HL.shard_range(n, rank, 2)
        p_r, rows_r, index_r = HL.prompt_table(path, n, lo, hi)
        assert p_r == prompts                                    # the prompts (and their numbering) do not depend on the rank
        assert [rows_r[i] for i in index_r] == [rows[i] for i in index[lo:hi]]      # every frame gets the row it has in the one-rank run
        assert sorted(set(index_r)) == list(range(len(rows_r)))                     # and the rank holds only the rows its frames use
        seen += [rows_r[i] for i in index_r]
    assert seen == [rows[i] for i in index]
    assert HL.shard_range(n, 0, 2) == (0, 3) and HL.prompt_table(path, n, 3, 5)[1] == [(1, 2, 0.5), (2, 2, 0.0)]


def test_example_config_loads():
    from tc_light_amd.config_utils import load_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        c = load_config(["--config", os.path.join("configs", "examples", "tclight_prompt_sweep.yaml")], print_config=False)
    finally:
        os.chdir(cwd)
    path = HL.check_prompt_path(c.generation.prompt_path, c.generation.get("normal", False), c.generation.get("highres_scale", 1.0))
    assert [p for p, _ in path] == [0.0, 0.5, 1.0] and c.generation.light_path == [[0, 0], [1, 180]]
    assert isinstance(c.generation.prompt, dict) and len(c.generation.prompt) == 1


# ---------------------------------------------------------------------------------------------------------------- run.py refuses before any model
@pytest.mark.parametrize("extra,words", [
    ("prompt_path: [[0, 'a'], [0.5, 'b']]", ["generation.prompt_path"]),
    ("prompt_path: [[0, 'a'], [1, 3]]", ["generation.prompt_path"]),
    ("prompt_path: [[0, 'a'], [1, 'b']]\n  highres_scale: 2.0", ["generation.prompt_path", "generation.highres_scale"]),
    ("prompt_path: [[0, 'a'], [1, 'b']]\n  normal: true\n  iclight_model: fbc\n  fbc_matting: false", ["generation.prompt_path", "generation.normal"]),
])
def test_run_refuses_before_models(tmp_path, monkeypatch, extra, words):
    import run
    import tc_light_amd.model_utils as M

    def boom(*a, **k):
        raise AssertionError("a model was loaded before generation.prompt_path was checked")
    monkeypatch.setattr(run, "init_iclight", boom)
    monkeypatch.setattr(M, "init_iclight", boom)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"""base_config: {os.path.join(ROOT, 'configs', 'tclight_default.yaml')}
work_dir: {tmp_path / 'work'}
data: {{height: 64, width: 64}}
generation:
  prompt: {{edit: "warm light"}}
  {extra}
""")
    with pytest.raises(ValueError) as e:
        run.main(["--config", str(cfg)])
    for w in words:
        assert w in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- the float sequence of the blend
T_SET = (0.0, 1.0, 0.5, 1.0 / 3.0)


def test_lerp_reference_is_the_stated_f32_sequence():
    keys = PR.make_keys(3, 7, 24, seed=3)
    rows = [(0, 1, t) for t in T_SET] + [(2, 0, 1.0 / 3.0), (1, 2, 0.75), (1, 1, 0.3), (2, 1, 1e-8), (0, 2, 1.0 - 2.0 ** -24)]
    want, got = PR.lerp_rows_f32(keys, rows), PR.lerp_rows(keys, rows)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # t = 0 and t = 1 are the keyframes' own bits, -0 and subnormals included (the formula alone gives +0 for a = -0, b - a = 0)
    assert np.array_equal(got[0].view(np.uint16), keys[0].view(np.uint16)) and np.array_equal(got[1].view(np.uint16), keys[1].view(np.uint16))
    assert (keys[0].view(np.uint16) == 0x8000).any() and (keys[0].view(np.uint16) == 0x0001).any()
    # hand-checked elements of the sequence
    k = np.array([[1.0, -65504.0, 2.0 ** -24, 3.0], [2.0, 65504.0, -2.0 ** -24, 3.0]], dtype=np.float16)
    (half, third), = [PR.lerp_rows(k, [(0, 1, 0.5), (0, 1, 1.0 / 3.0)])]
    assert half.tolist() == [1.5, 0.0, 0.0, 3.0]
    t3 = float(np.float32(1.0 / 3.0))
    assert third[0] == np.float16(np.float32(np.float32(1.0) + np.float32(t3 * 1.0))) and third[3] == 3.0
    assert third[2] == np.float16(np.float32(2.0 ** -24) + np.float32(np.float32(t3) * np.float32(-2.0 ** -23)))


def test_lerp_sequence_stays_within_half_an_ulp_of_the_real_blend():
    """The stated sequence against a + t (b - a) in float64, on unit-normal embeddings.  The three f32 roundings (of e, m and s) each err by at most
    2^-24 of a value no larger than |a| + |b|, so the f32 sum is within 3 * 2^-24 (|a| + |b|) of the real blend; the one f16 rounding adds half an
    f16 ulp of the result."""
    g = np.random.default_rng(11)
    keys = g.standard_normal((2, 4096)).astype(np.float16)
    for t in (0.5, 1.0 / 3.0, 0.9):
        got = PR.lerp_rows(keys, [(0, 1, t)])[0].astype(np.float64)
        a, b = keys[0].astype(np.float64), keys[1].astype(np.float64)
        exact = a + float(np.float32(t)) * (b - a)
        ulp = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(exact), 2.0 ** -14))) - 10), 2.0 ** -24)
        assert (np.abs(got - exact) <= 0.5 * ulp + 3 * 2.0 ** -24 * (np.abs(a) + np.abs(b))).all()


def test_t_bits_round_f64_to_f32_once():
    assert PR.t_bits(0.0) == 0 and PR.t_bits(1.0) == 0x3F800000 and PR.t_bits(0.5) == 0x3F000000
    assert PR.t_bits(1.0 / 3.0) == 0x3EAAAAAB
    import struct
    for t in (1.0 / 3.0, 0.25 / 0.3, 0.1, 1.0 - 2.0 ** -30):      # Generator.frame_text packs the table with struct: the same rounding
        assert struct.unpack("<i", struct.pack("<f", t))[0] == PR.t_bits(t)
