"""float64 restatements of the opset-23 operators Attention and RMSNormalization as the kernels serve them (hip/attention.hip with Tq != Tk,
grouped heads and is_causal; hip/layernorm.hip rmsnorm_kernel; INTEGRATION.md section 2.6 "The Attention operator", "RMSNormalization"),
float32 numpy restatements of the same formulas, and the shape lists of tests/test_attention_op_gpu.py.  numpy only:
tests/test_attention_op_ref.py checks this module without a GPU (against torch float64), the GPU test compares the kernels with it.

The verdict rule, the exact-score inputs and the LayerNorm input families are those of tests/attention_ref.py; the score of (query i, key j)
is rounded to float32 at the two places of the operator's definition there as well: fl32(scale . q_i . k_j), then fl32(that + mask[i, j]).
Exclusions (is_causal: j > i; a bool mask entry that is false; a row's own key mask) are a score of -inf: a weight of exactly 0.

Grouped heads: query head g reads K / V head g // (hq // hkv) -- repeat_interleave, which is what torch's exporter writes for its own
fallback and what torch computes on the CPU (test_attention_op_ref.py); is_causal with Tq != Tk is aligned top-left, torch's tril."""
from __future__ import annotations

import numpy as np

from tests import attention_ref as A

verdict, exact_case, unit_case, ln_inputs = A.verdict, A.exact_case, A.unit_case, A.ln_inputs
f32 = np.float32


def heads_of(a, h):
    N, T, Em = a.shape
    return a.reshape(N, T, h, Em // h).transpose(0, 2, 1, 3)


def excluded(Tq, Tk, causal=False, mask=None, keep=None, rows=1):
    """[rows, 1, Tq, Tk] bool: the keys a query does not see"""
    ex = np.zeros((rows, 1, Tq, Tk), bool)
    if causal:
        ex |= np.arange(Tk)[None, :] > np.arange(Tq)[:, None]
    if mask is not None and np.asarray(mask).dtype == np.bool_:
        ex |= ~np.broadcast_to(np.asarray(mask).reshape(np.shape(mask)[-2:]), (Tq, Tk))
    if keep is not None:
        ex |= ~np.asarray(keep, bool).reshape(rows, 1, 1, Tk)
    return ex


def additive(mask, Tq, Tk):
    """a float mask as its [Tq, Tk] table (float64), None for none or a bool mask"""
    if mask is None or np.asarray(mask).dtype == np.bool_:
        return None
    mk = np.asarray(mask, np.float32)
    return np.broadcast_to(mk.reshape(mk.shape[-2:]), (Tq, Tk)).astype(np.float64)


def attention(q, k, v, hq: int, hkv: int, scale: float, causal=False, mask=None, keep=None) -> np.ndarray:
    """q [N, Tq, hq dh], k, v [N, Tk, hkv dh] -> [N, Tq, hq dh] in float64 with the two f32 roundings of the score.  IEEE all the way, as
    attention_ref.attention: every product of P V is formed, so 0 . NaN = NaN."""
    N, Tq, Eq = np.shape(q)
    Tk, g = np.shape(k)[1], hq // hkv
    qh = heads_of(np.asarray(q, np.float64), hq)
    kh, vh = (np.repeat(heads_of(np.asarray(a, np.float64), hkv), g, axis=1) for a in (k, v))
    with np.errstate(all="ignore"):
        s = (np.einsum("nhqd,nhkd->nhqk", qh, kh) * float(scale)).astype(np.float32).astype(np.float64)
        mk = additive(mask, Tq, Tk)
        if mk is not None:
            s = (s + mk).astype(np.float32).astype(np.float64)
        s = np.where(excluded(Tq, Tk, causal, mask, keep, N), -np.inf, s)
        s = s - np.max(s, axis=-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(axis=-1, keepdims=True)
        out = np.einsum("nhqk,nhkd->nhqd", p, vh)
    return out.transpose(0, 2, 1, 3).reshape(N, Tq, Eq)


def attention32(q, k, v, hq: int, hkv: int, scale: float, causal=False, mask=None, keep=None) -> np.ndarray:
    """the same formula in float32 numpy throughout (not the kernel's order): what float32 itself costs on a case"""
    N, Tq, Eq = np.shape(q)
    Tk, g = np.shape(k)[1], hq // hkv
    qh = heads_of(np.asarray(q, np.float32), hq)
    kh, vh = (np.repeat(heads_of(np.asarray(a, np.float32), hkv), g, axis=1) for a in (k, v))
    with np.errstate(all="ignore"):
        s = np.matmul(qh, kh.transpose(0, 1, 3, 2)) * f32(scale)
        mk = additive(mask, Tq, Tk)
        if mk is not None:
            s = s + mk.astype(np.float32)
        s = np.where(excluded(Tq, Tk, causal, mask, keep, N), f32(-np.inf), s)
        s = s - np.max(s, axis=-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(axis=-1, keepdims=True, dtype=np.float32)
        out = np.matmul(p, vh)
    return out.astype(np.float32).transpose(0, 2, 1, 3).reshape(N, Tq, Eq)


def rmsnorm(x, g, eps) -> np.ndarray:
    """x / sqrt(mean(x^2) + eps) . gamma over the last axis in float64; eps as the f32 the kernel holds"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + np.float64(np.float32(eps))) * np.asarray(g, np.float64)


def rmsnorm32(x, g, eps) -> np.ndarray:
    """the documented formula in float32 numpy: y = x / sqrtf(sum(x^2) / E + eps) . gamma.  numpy's sum is pairwise, the kernel's a butterfly
    over per-lane partial sums: the same formula, not the same bits."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        ms = (x * x).sum(axis=-1, keepdims=True, dtype=np.float32) / f32(x.shape[-1])
        return x / np.sqrt(ms + f32(eps)) * np.asarray(g, np.float32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

POW2_SCALE = {5: 0.5, 16: 0.25, 40: 0.125, 64: 0.125}  # a power of two per head width: exact scores on the integer grid (attention_ref)


def case(kind: str, Tq: int, Tk: int, hq: int, hkv: int, dh: int, rows: int, seed: int = 0):
    """(q [rows, Tq, hq dh], k, v [rows, Tk, hkv dh]) float32.  kind "unit": uniform(-1, 1); "exact": the integer grid "unit" of
    attention_ref.exact_case (scores exact in float32 under POW2_SCALE[dh]).  Drawn for max(Tq, Tk) steps and hq heads, then cut: a
    subset of exact scores is exact."""
    T = max(Tq, Tk)
    if kind == "unit":
        q, k, v = unit_case(T, hq * dh, rows, seed=seed)
    else:
        q, k, v = exact_case(T, dh, hq, rows, "unit", POW2_SCALE[dh], seed=seed)
    cut = lambda a, t, h: np.ascontiguousarray(a[:, :t, :h * dh])  # noqa: E731
    return cut(q, Tq, hq), cut(k, Tk, hkv), cut(v, Tk, hkv)


def table(q, k, v, cols=None):
    """the call's table: Q, K, V flattened one after the other, then the mask's columns"""
    rows = q.shape[0]
    parts = [a.reshape(rows, -1) for a in (q, k, v)] + ([] if cols is None else [np.asarray(cols, np.float32)])
    return np.ascontiguousarray(np.concatenate(parts, axis=1), np.float32)


def repeat_kv(a, hkv: int, g: int):
    """[N, T, hkv dh] -> [N, T, hkv g dh]: every head g times in a row (repeat_interleave)"""
    N, T, Em = a.shape
    return np.ascontiguousarray(np.repeat(a.reshape(N, T, hkv, Em // hkv), g, axis=2).reshape(N, T, Em * g))


def right_padded(lengths, Tk):
    """keep [rows, Tk]: row r keeps keys [0, lengths[r])"""
    return np.arange(Tk)[None, :] < np.asarray(lengths)[:, None]


# ---- the shape lists of tests/test_attention_op_gpu.py ---------------------------------------------------------------------------------

ROWS = 7
CAUSAL_T = (1, 16, 17, 33, 64, 65, 129)
CAUSAL_DH = (5, 16, 40, 64)
CAUSAL_H = 2
GROUPS = ((4, 2), (6, 1), (3, 3))  # (hq, hkv)
GROUP_SHAPE = (33, 16)             # T, dh
CROSS = tuple((tq, tk) for tq in (1, 15, 33) for tk in (33, 65, 100) if tq < tk)
CROSS_SHAPE = (2, 16)              # h, dh
LONGER_Q = ((33, 17), (65, 32))    # Tq > Tk, causal: queries >= Tk see every key
PADDED_CAUSAL_T = 33


def padded_lengths(Tk):
    return [0, 1, 16, 17, Tk, Tk // 2, 2]  # ROWS rows


# every configuration the float64 test walks: (Tq, Tk, hq, hkv, dh, causal, padded)
F64_CASES = ([(T, T, CAUSAL_H, CAUSAL_H, dh, True, False) for T in CAUSAL_T for dh in CAUSAL_DH]
             + [(GROUP_SHAPE[0], GROUP_SHAPE[0], hq, hkv, GROUP_SHAPE[1], c, False) for hq, hkv in GROUPS for c in (False, True)]
             + [(tq, tk, CROSS_SHAPE[0], CROSS_SHAPE[0], CROSS_SHAPE[1], c, False) for tq, tk in CROSS for c in (False, True)]
             + [(tq, tk, 4, 2, 16, True, False) for tq, tk in LONGER_Q]
             + [(PADDED_CAUSAL_T, PADDED_CAUSAL_T, 4, 2, 16, True, True)])
F64_ID = lambda c: "Tq%d_Tk%d_h%d_kv%d_dh%d%s%s" % (c[0], c[1], c[2], c[3], c[4], "_causal" if c[5] else "", "_padded" if c[6] else "")  # noqa: E731

RMS_EPS = 1e-5
