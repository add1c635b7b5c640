"""The cases of tests/test_spatial_norm_range_gpu.py and what proves that they reach every launch form of hip/spatialnorm.hip, without a
GPU: the ladder of launch_fused_by_size and the unit rule of host/spatialnorm.cpp restated (rung_of, unit_of: labels and the coverage
proof of tests/test_spatial_norm_cases.py, never an input of the kernel), the case table, the inputs at the value edges (value_inputs) and
the kernel's documented arithmetic (the header of host/spatialnorm.hpp) in numpy float32 (emulate_f32), which shows that those inputs can
meet the parity bar of DESIGN.md section 5 at all -- not what the device computes bit for bit."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

FUSED_MAX = 16384  # host/spatialnorm.hpp kSpatialNormFusedMaxE
RTOL, ATOL = 1e-4, 1e-6

# launch_fused_by_size: (largest U, lanes per unit L, quads per lane NV)
LADDER = [(32, 8, 1), (64, 16, 1), (128, 32, 1), (256, 64, 1), (1024, 64, 4), (4096, 64, 16), (FUSED_MAX, 256, 16)]
RUNGS = [(l, nv) for _, l, nv in LADDER]
BOUNDARIES = [top for top, _, _ in LADDER]


def rung_of(u: int) -> tuple[int, int]:
    """(L, NV) of the instantiation that a fused unit of u floats runs on"""
    assert 1 <= u <= FUSED_MAX, u
    return next((l, nv) for top, l, nv in LADDER if u <= top)


def unit_of(c: int, g: int, s: int, cq: bool):
    """spatialnorm_fused_unit: (mode, U) of a layer of c channels in g groups over s positions, on an NCHW (cq False) or channel-quad
    tensor; None: the general plan.  Mode 0: one group per unit; mode 1: one quad plane [s][4] of four groups or of two."""
    cg = c // g
    if not cq or s == 1 or cg % 4 == 0:
        return (0, cg * s) if cg * s <= FUSED_MAX else None
    if cg in (1, 2):
        return (1, 4 * s) if 4 * s <= FUSED_MAX else None
    return None


NCHW, CQ = "nchw_in_nchw_out", "cq_in_cq_out"
LAYOUTS = {NCHW: dict(pre=False, post=False), CQ: dict(pre=True, post=True)}  # (tests/test_spatial_norm_gpu.py)


class Case(NamedTuple):
    name: str
    c: int
    g: int
    hw: tuple
    layout: str
    plan: str          # "default", or "general": loaded under INFERA_SPATIALNORM_FUSED=0
    fused: bool        # whether the planner must choose spatialnorm_fused
    rows: tuple
    light: bool        # the two grid-stride cases: once, without an activation

    @property
    def s(self) -> int:
        return int(np.prod(self.hw))

    @property
    def e(self) -> int:
        return (self.c // self.g) * self.s

    @property
    def unit(self):
        return unit_of(self.c, self.g, self.s, self.layout == CQ)

    @property
    def label(self):
        """(mode, L, NV) of a case on the fused kernel, None on the general plan"""
        u = self.unit
        return None if u is None or self.plan == "general" else (u[0],) + rung_of(u[1])


def _rows(c, g, s, cq):
    """(1, 3, 70) where the work unit has at most 4100 floats, (1, 3) above"""
    u = unit_of(c, g, s, cq)
    size = u[1] if u else (4 * s if cq and s > 1 and (c // g) % 4 else (c // g) * s)
    return (1, 3, 70) if size <= 4100 else (1, 3)


def _case(c, g, hw, layout, plan="default", fused=True, rows=None, light=False):
    hw = tuple(hw)
    s = int(np.prod(hw))
    name = f"{'nchw' if layout == NCHW else 'cq'}_c{c}_g{g}_{'x'.join(map(str, hw))}" + ("_general" if plan == "general" else "")
    return Case(name, c, g, hw, layout, plan, fused and plan == "default", rows or _rows(c, g, s, layout == CQ), light)


def _table():
    t = []
    # NCHW, mode 0, C = G = 3: three units per row, so the last workgroup has idle unit slots at every L < 256; both sides of every boundary
    for u in (32, 33, 64, 65, 128, 129, 256, 257, 1024, 1025, 4096, 4097, 16383, 16384):
        t.append(_case(3, 3, (u,), NCHW))
    t.append(_case(3, 3, (16385,), NCHW, fused=False))
    # channel quads, mode 1, C = G = 4: U = 4 S
    for s in (8, 9, 16, 17, 32, 33, 64, 65, 256, 257, 1024, 1025, 4096):
        t.append(_case(4, 4, (s,), CQ))
    t.append(_case(4, 4, (4097,), CQ, fused=False))
    # mode 1 with two channels per group: components (0, 1) and (2, 3) are added after the lanes are joined
    for s in (8, 65, 1025, 4096):
        t.append(_case(8, 4, (s,), CQ))
    # mode 0 on channel quads: whole quad planes per group; C / G = 8: a unit spans two planes
    for s in (8, 257, 1024):
        t.append(_case(8, 2, (s,), CQ))
    t.append(_case(16, 2, (65,), CQ))
    # S = 1: the same floats in either layout, the channel-quad indexing is off; (8, 8): E = 1
    for c, g in ((32, 8), (8, 8), (12, 4)):
        for layout in (NCHW, CQ):
            t.append(_case(c, g, (1, 1), layout))
    # the general plan: groups that straddle quads with two steps of the stats loop; the element loop of the stats kernel twice; the
    # apply kernel's grid-stride loop (8192 blocks of 256 lanes) a second time, by elements and by quads
    t.append(_case(12, 4, (10, 10), CQ, fused=False))
    t.append(_case(3, 3, (17, 17), NCHW, plan="general"))
    t.append(_case(1, 1, (255, 257), NCHW, fused=False, rows=(33,), light=True))
    t.append(_case(1, 1, (256, 256), NCHW, fused=False, rows=(129,), light=True))
    return t


TABLE = _table()
BY_NAME = {k.name: k for k in TABLE}
assert len(BY_NAME) == len(TABLE)


def _pick(*names):
    return [BY_NAME[n].name for n in names]


# test_value_edges: one case per rung and mode, and the general cases that are not there for their size alone
EDGE_CASES = _pick(
    "nchw_c3_g3_32", "nchw_c3_g3_33", "nchw_c3_g3_65", "nchw_c3_g3_129", "nchw_c3_g3_257", "nchw_c3_g3_1025", "nchw_c3_g3_16383",  # mode 0
    "cq_c4_g4_8", "cq_c4_g4_9", "cq_c4_g4_17", "cq_c4_g4_33", "cq_c4_g4_65", "cq_c4_g4_257", "cq_c4_g4_4096",                       # mode 1
    "cq_c8_g4_65", "cq_c8_g4_1025",                                                                                                # cg = 2
    "cq_c8_g2_8", "cq_c16_g2_65", "cq_c8_g2_257",                                                                                  # mode 0, quads
    "cq_c12_g4_1x1", "cq_c12_g4_10x10", "nchw_c3_g3_17x17_general", "nchw_c3_g3_16385", "cq_c4_g4_4097")
# test_groups_do_not_see_each_other: several groups per unit or per wave
NEIGHBOUR_CASES = [_case(3, 3, (19,), NCHW)] + [BY_NAME[n] for n in _pick(
    "nchw_c3_g3_33", "nchw_c3_g3_65", "nchw_c3_g3_257", "cq_c4_g4_8", "cq_c4_g4_65", "cq_c4_g4_1025", "cq_c8_g4_8", "cq_c8_g4_65",
    "cq_c8_g4_1025", "cq_c12_g4_10x10")]

# ---- inputs at the value edges -------------------------------------------------------------------------------------------------------
# kind -> (scale of U(-1, 1), epsilon).  "small": the variance, about 3e-13, is comparable to epsilon; "eps_rules": epsilon is about 30
# times the variance; "outlier": one element of every group is 1e4 -- the first mean is then far from most elements.
VALUE_KINDS = {"big": (2.0 ** 40, 1e-5), "small": (2.0 ** -20, 1e-12), "eps_rules": (2.0 ** -10, 1e-5), "outlier": (1.0, 1e-5)}
OUTLIER = 1e4


def value_groups(n_groups: int, e: int, kind: str, seed: int, offset: float = 0.0) -> np.ndarray:
    """[n_groups, e] float32 of `kind`, one row per normalisation group"""
    scale, _ = VALUE_KINDS[kind]
    rng = np.random.default_rng(seed)
    x = scale * rng.uniform(-1, 1, size=(n_groups, e))
    if kind == "outlier":
        x[np.arange(n_groups), rng.integers(0, e, size=n_groups)] = OUTLIER
    return (offset + x).astype(np.float32)


def value_inputs(spec: dict, rows: int, kind: str, seed: int = 0):
    """(x [rows, C, ...] float32, epsilon) for a spec of onnx_writer.spatial_norm_model, which must have been built with that epsilon;
    spec["offset"] is added to every element"""
    p = next(p for op, out, ins, p in spec["layers"] if out == "norm")
    eps = VALUE_KINDS[kind][1]
    assert p["eps"] == float(np.float32(eps)), (p["eps"], eps)
    shape = tuple(spec["in_shape"])
    g = p["groups"]
    x = value_groups(rows * g, int(np.prod(shape)) // g, kind, seed, spec.get("offset", 0.0))
    return x.reshape((rows,) + shape), eps


# ---- the documented arithmetic in float32 ----------------------------------------------------------------------------------------------
def _pairwise(v: np.ndarray) -> np.ndarray:
    """[n, lanes] -> [n]: neighbours joined pairwise, the shape of the xor butterfly and of (w0 + w1) + (w2 + w3); each sum rounded"""
    assert v.dtype == np.float32
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _lane_sum(v: np.ndarray, lanes: int, by_quads: bool) -> np.ndarray:
    """[n, e] -> [n]: lane l sums quads (by_quads) or elements l, l + lanes, ... in that order, then the lanes are joined pairwise"""
    n, e = v.shape
    width = 4 if by_quads else 1
    steps = -(-e // (lanes * width))
    pad = np.zeros((n, steps * lanes * width), np.float32)
    pad[:, :e] = v
    pad = pad.reshape(n, steps, lanes, width)
    acc = np.zeros((n, lanes), np.float32)
    for q in range(steps):
        for j in range(width):
            acc = acc + pad[:, q, :, j]
    return _pairwise(acc)


def emulate_f32(x_groups, gamma, beta, eps, general: bool) -> np.ndarray:
    """y [n, E] float32 for x_groups [n, E] (one group per row) and gamma, beta that broadcast against it, every operation rounded to
    float32.  The fused form: the lanes of the group's rung take quads l, l + L, ...; d = x - mean, d -= sum(d) / E,
    y = d / sqrtf(sum(d^2) / E + eps) * gamma + beta.  The general form: 256 lanes, resid and var from one pass over d = x - mean,
    var = sum(d^2) / E - resid^2, y = ((x - mean) - resid) * (1 / sqrtf(var + eps)) * gamma + beta."""
    f = np.float32
    x = np.ascontiguousarray(x_groups, f)
    e = x.shape[1]
    gamma, beta, eps, n = np.asarray(gamma, f), np.asarray(beta, f), f(eps), f(e)
    lanes = 256 if general or e > 4096 else rung_of(e)[0]
    total = lambda v: _lane_sum(v, lanes, by_quads=not general or e % 4 == 0)[:, None]  # noqa: E731
    mean = total(x) / n
    d = x - mean
    resid = total(d) / n
    if general:
        var = total(d * d) / n - resid * resid
        inv = f(1.0) / np.sqrt(var + eps)
        y = (d - resid) * inv * gamma + beta
    else:
        d = d - resid
        den = np.sqrt(total(d * d) / n + eps)
        y = d / den * gamma + beta
    assert y.dtype == f
    return y


def reference_f64(x_groups, gamma, beta, eps) -> np.ndarray:
    x = np.asarray(x_groups, np.float64)
    d = x - x.mean(axis=1, keepdims=True)
    return d / np.sqrt((d * d).mean(axis=1, keepdims=True) + float(eps)) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def bar_ratio(got, want) -> float:
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64).reshape(want.shape) - want) / (RTOL * np.abs(want) + ATOL)).max())
