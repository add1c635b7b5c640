"""Shared by tests/test_deconv.py and tests/test_deconv_gpu.py: the transposed-convolution geometries, and the models around them."""
from __future__ import annotations

import numpy as np

from infera_amd import onnx_writer as W

# k, s (strides), p (pads: top, left, bottom, right), d (dilations), g (groups; "C": depthwise), op (output_padding)
GEOMETRIES = {
    "k2_s2": dict(k=2, s=2),
    "k3_s2_p1_op1": dict(k=3, s=2, p=1, op=1),
    "k4_s2_p1": dict(k=4, s=2, p=1),
    "k1_s2": dict(k=1, s=2),
    "k3_s1_p1": dict(k=3, s=1, p=1),
    "k3_s23_pads0121": dict(k=3, s=(2, 3), p=(0, 1, 2, 1)),
    "k3_s2_d2": dict(k=3, s=2, d=2),
    "groups4": dict(k=3, s=2, p=1, g=4),
    "depthwise": dict(k=3, s=2, p=1, g="C"),
}


def geometry(name: str, C: int, M: int, H: int | None, Wd: int) -> dict:
    g = dict(GEOMETRIES[name], C=C, M=M, W=Wd)
    if H is not None:
        g["H"] = H
    if g.get("g") == "C":
        g["g"], g["M"] = C, C
    return g


def out_extent(n_in, k, s, p0, p1, d, op):
    return (n_in - 1) * s - p0 - p1 + d * (k - 1) + op + 1


def expected_out_hw(g: dict) -> tuple:
    (kh, kw), (sh, sw), (dh, dw), (oph, opw) = (W._pair(g.get(k, v)) for k, v in (("k", 2), ("s", 2), ("d", 1), ("op", 0)))
    pt, pl, pb, pr = W._pads4(g.get("p", 0))
    if "H" not in g:  # 1-D: the H axis of the [N, C, 1, L] form is left alone
        return 1, out_extent(g["W"], kw, sw, pl, pr, dw, opw)
    return out_extent(g["H"], kh, sh, pt, pb, dh, oph), out_extent(g["W"], kw, sw, pl, pr, dw, opw)


def small_ints(seed: int, shape) -> np.ndarray:
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float32)
