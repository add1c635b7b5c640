"""References and shape lists for the Rotary step (hip/rotary.hip; INTEGRATION.md section 2.6 "Rotary position embeddings").

The step's definition over a window x [N, T, h dh] with two float32 factor tables A, B [T, rd]: for column j < rd of every head

    out[j] = fl(fl(x[j] A[t, j]) + fl(x[partner(j)] B[t, j]))          partner(j) = j +- rd / 2 (half) or j ^ 1 (interleaved)

three separately rounded float32 operations; columns j >= rd are bit copies.  step32 evaluates exactly that (numpy rounds every float32
operation once), step64 the same formula in float64 on the same float32 tables.  Both are written pair by pair, independently of the
writer's rotary_reference, which the tests compare them with.

Inputs.  The project's bar is 1e-4 |ref| + 1e-6 per element.  The definition's error is at most
2^-24 (|x[j] A| + |x[p] B| + |out|) <= 2^-24 (2 sqrt 2) max|x| (A, B are a cosine and a sine of one angle), and where the two products cancel
the bar is its absolute term 1e-6: a quarter of the bar needs max|x| <= 1.4.  So the families keep |x| <= 1: "unit" uniform(-1, 1) -- what
the attention tests feed -- and "tenth" uniform(-0.1, 0.1).  Inputs of magnitude 100 would miss a quarter of the bar by the definition's own
rounding; they are used for bit comparisons only."""
from __future__ import annotations

import numpy as np

from tests import attention_ref as A

verdict = A.verdict
ROWS = 7


def tables(T: int, rd: int, base: float = 10000.0, positions=None):
    """cos, sin [T, rd / 2] float32: angles in float64, rounded once"""
    pos = np.arange(T, dtype=np.float64) if positions is None else np.asarray(positions, np.float64)
    inv = np.array([base ** (-2.0 * i / rd) for i in range(rd // 2)], dtype=np.float64)
    ang = np.outer(pos, inv)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def factors(cos, sin, interleaved: bool):
    """A, B [T, rd] of cos, sin [T, rd / 2]"""
    T, half = cos.shape
    Af, Bf = np.empty((T, 2 * half), np.float32), np.empty((T, 2 * half), np.float32)
    for i in range(half):
        a, b = (2 * i, 2 * i + 1) if interleaved else (i, i + half)
        Af[:, a] = Af[:, b] = cos[:, i]
        Bf[:, a], Bf[:, b] = -sin[:, i], sin[:, i]
    return Af, Bf


def _step(x, Af, Bf, h, dh, interleaved, dtype):
    x = np.asarray(x, dtype=dtype)
    N, T = x.shape[:2]
    rd = Af.shape[1]
    x4 = x.reshape(N, T, h, dh)
    out = x4.copy()
    Af, Bf = np.asarray(Af, dtype)[None, :, None, :], np.asarray(Bf, dtype)[None, :, None, :]
    with np.errstate(all="ignore"):
        for i in range(rd // 2):
            a, b = (2 * i, 2 * i + 1) if interleaved else (i, i + rd // 2)
            out[..., a] = x4[..., a] * Af[..., a] + x4[..., b] * Bf[..., a]
            out[..., b] = x4[..., b] * Af[..., b] + x4[..., a] * Bf[..., b]
    return out.reshape(N, T, h * dh)


def step32(x, Af, Bf, h, dh, interleaved=False):
    return _step(x, Af, Bf, h, dh, interleaved, np.float32)


def step64(x, Af, Bf, h, dh, interleaved=False):
    return _step(x, Af, Bf, h, dh, interleaved, np.float64)


def rope32(x, T, h, dh, rd=0, interleaved=False, positions=None, cache=None):
    """the operator over x [N, T, h dh] in the step's float32 arithmetic; positions / cache = (cos, sin): rows gathered from a cache"""
    rd = rd or dh
    cos, sin = tables(T, rd) if cache is None else (cache[0][positions], cache[1][positions])
    return step32(x, *factors(cos, sin, interleaved), h, dh, interleaved)


def rope64(x, T, h, dh, rd=0, interleaved=False):
    rd = rd or dh
    return step64(x, *factors(*tables(T, rd), interleaved), h, dh, interleaved)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

FAMILIES = ("unit", "tenth")


def inputs(family: str, rows: int, T: int, E: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    scale = {"unit": 1.0, "tenth": 0.1, "hundred": 100.0}[family]  # ("hundred": bit comparisons only, see above)
    return (rng.uniform(-1, 1, (rows, T, E)) * scale).astype(np.float32)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------

STEP_DH = (2, 4, 6, 8, 10, 16, 64, 128)
STEP_H = (1, 3)
STEP_T = (1, 2, 5, 33)


def expected_form(dh: int, rd: int, interleaved: bool, ld: int | None = None, off: int = 0) -> str:
    """the form the host selects for a view: 16-byte loads need off, ld and dh multiples of 4 and rd / 2 (half) or rd (interleaved) too"""
    ok = dh % 4 == 0 and off % 4 == 0 and (ld is None or ld % 4 == 0) and (rd % 4 == 0 if interleaved else (rd // 2) % 4 == 0)
    return "vec4" if ok else "scalar"


def step_cases():
    """(dh, rd, interleaved, h, T): every dh with rd in {dh, dh / 2 where even, 2} in both pairings; h and T walk their lists so that each
    value meets both forms"""
    out, k = [], 0
    for dh in STEP_DH:
        rds = [dh] + ([dh // 2] if dh // 2 >= 2 and (dh // 2) % 2 == 0 else []) + ([2] if dh > 2 else [])
        for rd in dict.fromkeys(rds):
            for inter in (False, True):
                out.append((dh, rd, inter, STEP_H[(k // 2) % 2], STEP_T[k % 4]))
                k += 1
    return out


VIEW_SHAPES = ((3, 6), (2, 8))       # (h, dh) of the packed projection: K at column 18 (no 16-byte alignment) and at 16
SPELL_T = (1, 17, 129)
SPELL_DH = (16, 40)
SPELL_H = 2
PARITY_T = (1, 17, 129)
PARITY_HEADS = (4, 2)                # hq, hkv
PARITY_DH = 16
