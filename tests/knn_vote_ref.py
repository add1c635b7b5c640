"""numpy restatements of the k-NN vote (INTEGRATION.md section 2.6 "The k-NN vote"): vote_reference in float64, and vote_f32, which performs
exactly the f32 operations of hip/nearest.hip's nearest_vote_kernel in their order, so that its results are the kernel's BIT FOR BIT
whenever the neighbour lists agree.  The neighbours come from onnx_writer.nearest_reference (or from the search model of the same spec)."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def tol_of(ref: dict, F: int):
    """the bound of tests/test_nearest_gpu.py on a served d2: (F + 12) 2^-24 mag"""
    return (F + 12) * U * ref["mag"]


def first_max(v):
    """the ArgMax step's rule: element 0 starts the scan, a later element wins where it compares greater (a NaN never does; a NaN at 0 stays)"""
    v = np.asarray(v)
    best, at = v[:, 0].copy(), np.zeros(v.shape[0], np.int64)
    for c in range(1, v.shape[1]):
        with np.errstate(invalid="ignore"):
            up = v[:, c] > best
        best[up], at[up] = v[up, c], c
    return at


def vote_reference(neighbour_idx, neighbour_val, y=None, target=None, C: int = 0, weights: str = "uniform", eps: float = 1e-6) -> dict:
    """float64.  neighbour_idx [N, k]: the neighbours in ascending order; neighbour_val [N, k]: their distances AS THE GRAPH WEIGHTS THEM
    (rooted or not).  y [M] class indices with C classes -> `v` [N, C] class weights, `s` their sum, `proba`, `label` (class index, the
    first maximum); target [M] -> `value` [N] and `mag` = sum |w t| / sum w, the magnitude its rounding error scales with."""
    idx = np.asarray(neighbour_idx, np.int64)
    d = np.asarray(neighbour_val, np.float64)
    N, k = idx.shape
    with np.errstate(all="ignore"):
        w = np.ones((N, k)) if weights == "uniform" else 1.0 / np.maximum(d, np.float64(np.float32(eps)))  # (np.maximum keeps a NaN, as ONNX Max does)
        s = w.sum(1)
        out = {"w": w, "s": s}
        if y is not None:
            cls = np.asarray(y, np.int64)[idx]
            v = np.zeros((N, C))
            for j in range(k):
                v[np.arange(N), cls[:, j]] += w[:, j]
            out.update(v=v, proba=v / s[:, None], label=first_max(v))
        if target is not None:
            t = np.asarray(target, np.float64)[idx]
            out.update(value=(w * t).sum(1) / s, mag=np.abs(w * t).sum(1) / s)
    return out


def vote_f32(neighbour_idx, neighbour_d2, y=None, target=None, C: int = 0, weights: str = "uniform", eps: float = 1e-6, rooted: bool = True) -> dict:
    """The kernel's arithmetic: d = sqrtf(d2) when rooted; w = 1 or 1.f / fmaxf(d, eps) (one correctly rounded division; a NaN distance is a
    NaN weight); v_c, s and the regression sum run over ascending j from 0.f, every product rounded on its own; p_c = v_c / s; the label is
    the first maximum; uniform regression divides by float(k)."""
    f = np.float32
    idx = np.asarray(neighbour_idx, np.int64)
    d2 = np.asarray(neighbour_d2).astype(f)
    N, k = idx.shape
    with np.errstate(all="ignore"):
        d = np.sqrt(d2) if rooted else d2
        w = np.ones((N, k), f) if weights == "uniform" else (f(1.0) / np.maximum(d, f(eps))).astype(f)
        s = np.zeros(N, f)
        for j in range(k):
            s = (s + w[:, j]).astype(f)
        out = {"w": w, "s": s}
        if y is not None:
            cls = np.asarray(y, np.int64)[idx]
            v = np.zeros((N, C), f)
            rows = np.arange(N)
            for j in range(k):
                v[rows, cls[:, j]] = (v[rows, cls[:, j]] + w[:, j]).astype(f)
            out.update(v=v, proba=(v / s[:, None]).astype(f), label=first_max(v))
        if target is not None:
            t = np.asarray(target).astype(f)[idx]
            a = np.zeros(N, f)
            for j in range(k):
                a = (a + ((w[:, j] * t[:, j]).astype(f) if weights != "uniform" else t[:, j])).astype(f)
            out["value"] = (a / (s if weights != "uniform" else f(k))).astype(f)
    return out
