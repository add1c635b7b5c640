"""Per-row key masks (INTEGRATION.md section 2.6 "Padded sequences"): float64 restatements of attention and of the mean over time under a
row's own mask, and the length patterns the tests walk.  numpy only; tests/test_padded.py checks this module without a GPU,
tests/test_padded_gpu.py compares the kernels with it on one.  The attention is tests/attention_ref.py's, called row by row with that
row's [1, T] mask, so its two f32 roundings -- fl32(scale . q . k), then fl32(that + mask) -- are the ones the constant-mask tests use."""
from __future__ import annotations

import numpy as np

from tests import attention_ref as A

FMIN = A.FMIN
verdict = A.verdict


def attention_rows(q, k, v, h: int, scale: float, keep, fill: float, mode: str = "add") -> np.ndarray:
    """softmax over each row's keys with the row's own mask: q, k, v [N, T, E], keep [N, T] bool -> [N, T, E] float64.  mode "add": a
    masked key's rounded score is fl32(fl32(scale . q . k) + fill) (attention_ref.attention with the mask [1, T] = 0 / fill); "replace":
    it is `fill` itself.  A row without a kept key follows from the same arithmetic: equal scores where the fill absorbs them (uniform
    weights, the mean of V), NaN under -inf."""
    q, k, v = (np.asarray(a, np.float32) for a in (q, k, v))
    keep = np.asarray(keep, bool)
    N, T, Em = q.shape
    out = np.empty((N, T, Em), np.float64)
    b = np.float64(np.float32(fill))
    for r in range(N):
        qr, kr, vr = q[r:r + 1], k[r:r + 1], v[r:r + 1]
        if mode == "add":
            out[r] = A.attention(qr, kr, vr, h, scale, mask=np.where(keep[r], np.float32(0), np.float32(fill)).reshape(1, T))[0]
            continue
        assert mode == "replace", mode
        with np.errstate(all="ignore"):
            s = np.where(keep[r].reshape(1, 1, 1, T), A.rounded_scores(qr, kr, h, scale, None), b)
            s = s - np.max(s, axis=-1, keepdims=True)
            p = np.exp(s)
            p = p / p.sum(axis=-1, keepdims=True)
            o = np.einsum("nhqk,nhkd->nhqd", p, A.heads_of(vr.astype(np.float64), h))
        out[r] = o.transpose(0, 2, 1, 3).reshape(T, Em)
    return out


def masked_mean(x, keep, clip: float) -> np.ndarray:
    """[N, T, E], keep [N, T] -> [N, E] in float64: (the sum over the kept steps) / max(count, clip); a masked step is not read"""
    x, keep = np.asarray(x, np.float64), np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        s = np.where(keep[:, :, None], x, 0.0).sum(axis=1)
        return s / np.maximum(keep.sum(axis=1, keepdims=True).astype(np.float64), np.float64(np.float32(clip)))


# ---- length patterns ------------------------------------------------------------------------------------------------------------------

PAD_LENGTHS = (15, 16, 17, 31, 32, 33)
PATTERNS = ("all", "first", "last") + tuple("right%d" % n for n in PAD_LENGTHS) + ("right_random",) + tuple("left%d" % n for n in PAD_LENGTHS) + (
    "left_random", "holes", "tile")


def pattern(name: str, T: int, rng) -> np.ndarray:
    """one row's keep [T]; every pattern keeps at least one key.  rightL / leftL: L kept keys (clipped to T) at the start / the end, so a
    left-padded row starts with wholly masked sub-tiles and tiles; holes: every third key masked; tile: keys 32 .. 63 masked (T > 64; the
    middle third below that)."""
    keep = np.ones(T, bool)
    if name == "first":
        keep[1:] = False
    elif name == "last":
        keep[:-1] = False
    elif name.startswith("right") or name.startswith("left"):
        tail = name[5:] if name.startswith("right") else name[4:]
        L = min(T, int(rng.integers(1, T + 1)) if tail == "_random" else int(tail))
        keep[:] = False
        if name.startswith("right"):
            keep[:L] = True
        else:
            keep[T - L:] = True
    elif name == "holes":
        keep[1::3] = False
    elif name == "tile":
        if T > 64:
            keep[32:64] = False
        elif T >= 3:
            keep[T // 3:2 * T // 3] = False
    else:
        assert name == "all", name
    assert keep.any()
    return keep


def keep_rows(T: int, rows: int, seed: int = 0) -> np.ndarray:
    """keep [rows, T]: the patterns in order, again from the start when rows exceed them"""
    rng = np.random.default_rng([seed, T])
    return np.stack([pattern(PATTERNS[r % len(PATTERNS)], T, rng) for r in range(rows)])


def mask_columns(keep, source: str, pad_id: int, rng) -> np.ndarray:
    """the [rows, T] f32 columns a call passes for the mask: source "mask": 1 / 0; "ids": token ids, pad_id exactly at the masked steps"""
    keep = np.asarray(keep, bool)
    if source == "mask":
        return keep.astype(np.float32)
    ids = rng.integers(0, 1000, keep.shape)
    ids = np.where(ids == pad_id, pad_id + 1, ids)
    return np.where(keep, ids, pad_id).astype(np.float32)
