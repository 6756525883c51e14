"""Host restatement of tcl_text_lerp_f16 (include/tclight_hip.h), the blend of two keyframe prompts' embeddings under generation.prompt_path.

The stated sequence, per element, with a = keys[k0][i], b = keys[k1][i] (f16) and t the f64 blend factor rounded to f32 once:
    a32 = f32(a);  b32 = f32(b);  e = fl32(b32 - a32);  m = fl32(t * e);  s = fl32(a32 + m);  out = f16(s)
and t == 0 / t == 1 copy the f16 bits of keys[k0] / keys[k1].

`lerp_rows` computes it in float64 and rounds to f32 after every operation.  That IS the f32 operation: for +, -, * a result rounded first to 53 and
then to 24 bits equals the one rounded to 24 bits directly, because 53 >= 2 * 24 + 2 (the classical double-rounding condition); f32 operands are
exact in f64.  `lerp_rows_f32` is the same sequence in numpy float32 arithmetic; tests/test_prompt_path_host_cpu.py pins the two to each other."""
import numpy as np

F16_MAX = 65504.0
F16_MIN_SUBNORMAL = 2.0 ** -24


def f32(x):
    """Round a float64 array to the nearest f32 (ties to even), kept as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def lerp_rows(keys, rows):
    """keys [K, LD] np.float16; rows [(k0, k1, t)] -> [len(rows), LD] np.float16."""
    keys = np.asarray(keys)
    assert keys.dtype == np.float16
    out = np.empty((len(rows),) + keys.shape[1:], dtype=np.float16)
    for f, (k0, k1, t) in enumerate(rows):
        t32 = float(np.float32(t))
        if t32 == 0.0:
            out[f] = keys[k0]
        elif t32 == 1.0:
            out[f] = keys[k1]
        else:
            a = keys[k0].astype(np.float64)
            e = f32(keys[k1].astype(np.float64) - a)
            m = f32(t32 * e)
            s = f32(a + m)
            out[f] = s.astype(np.float32).astype(np.float16)
    return out


def lerp_rows_f32(keys, rows):
    """The same sequence in numpy float32 arithmetic (every operation IEEE-rounded to f32)."""
    keys = np.asarray(keys)
    out = np.empty((len(rows),) + keys.shape[1:], dtype=np.float16)
    for f, (k0, k1, t) in enumerate(rows):
        t32 = np.float32(t)
        if t32 == 0.0:
            out[f] = keys[k0]
        elif t32 == 1.0:
            out[f] = keys[k1]
        else:
            a = keys[k0].astype(np.float32)
            e = keys[k1].astype(np.float32) - a
            m = t32 * e
            out[f] = (a + m).astype(np.float16)
    return out


def make_keys(n_keys, L, D, seed):
    """n_keys embeddings [n_keys, L*D] f16: unit normals, with f16 subnormals, +-0, +-max and the smallest normals planted at the same places of
    every key in rotating order, so that every pair of keys meets every combination of them somewhere."""
    g = np.random.default_rng(seed)
    keys = g.standard_normal((n_keys, L * D)).astype(np.float16)
    special = np.array([F16_MIN_SUBNORMAL, -F16_MIN_SUBNORMAL, 1023 * F16_MIN_SUBNORMAL, -5 * F16_MIN_SUBNORMAL, 0.0, -0.0, F16_MAX, -F16_MAX,
                        2.0 ** -14, -2.0 ** -14, 1.0, -1.0], dtype=np.float16)
    n = len(special)
    for k in range(n_keys):
        for shift in range(min(n, (L * D - n) // n)):      # block `shift` of n elements: key k holds special rotated by k * shift
            keys[k, shift * n:(shift + 1) * n] = np.roll(special, k * shift)
        keys[k, -n:] = np.roll(special, k)           # and at the very end of the row (the last lanes of the last block)
    return keys


def t_bits(t):
    """The int32 whose bits are f32(t): what the table of tcl_text_lerp_f16 carries."""
    return int(np.array([t], dtype=np.float32).view(np.int32)[0])
