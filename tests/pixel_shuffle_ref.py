"""numpy reference of the four sub-pixel forms (INTEGRATION.md 2.6 "Sub-pixel layers"), written from the index formulas alone: every output
element is looked up through index arrays, nothing is reshaped or transposed.  With block size b, i, j in [0, b) and k = i b + j:

    dcr        y[n, c, h b + i, w b + j] = x[n, k C' + c, h, w]     (DepthToSpace, mode DCR; C' = C / b^2)
    crd        y[n, c, h b + i, w b + j] = x[n, c b^2 + k, h, w]    (DepthToSpace, mode CRD = torch's pixel_shuffle)
    s2d        y[n, k C + c, h, w] = x[n, c, h b + i, w b + j]      (SpaceToDepth)
    unshuffle  y[n, c b^2 + k, h, w] = x[n, c, h b + i, w b + j]    (torch's pixel_unshuffle)

The values are moved, never computed with: the result has x's dtype and x's bits."""
from __future__ import annotations

import numpy as np

FORMS = ("dcr", "crd", "s2d", "unshuffle")
TO_SPACE = ("dcr", "crd")


def out_shape(form: str, b: int, c: int, h: int, w: int) -> tuple:
    return (c // (b * b), h * b, w * b) if form in TO_SPACE else (c * b * b, h // b, w // b)


def source_index(form: str, b: int, c: int, h: int, w: int):
    """For every output element (oc, oh, ow): the input element (c, y, x) it copies, as three integer arrays of the output's shape."""
    oc_n, oh_n, ow_n = out_shape(form, b, c, h, w)
    oc, oh, ow = np.meshgrid(np.arange(oc_n), np.arange(oh_n), np.arange(ow_n), indexing="ij")
    if form in TO_SPACE:
        k = (oh % b) * b + ow % b
        src_c = k * oc_n + oc if form == "dcr" else oc * b * b + k
        return src_c, oh // b, ow // b
    if form == "s2d":
        k, src_c = oc // c, oc % c
    elif form == "unshuffle":
        k, src_c = oc % (b * b), oc // (b * b)
    else:
        raise ValueError(form)
    return src_c, oh * b + k // b, ow * b + k % b


def pixel_shuffle(x, form: str, b: int) -> np.ndarray:
    x = np.asarray(x)
    n, c, h, w = x.shape
    if b < 1 or (form in TO_SPACE and c % (b * b)) or (form not in TO_SPACE and (h % b or w % b)):
        raise ValueError((form, b, x.shape))
    sc, sy, sx = source_index(form, b, c, h, w)
    return x[:, sc, sy, sx]


def pixel_shuffle_loops(x, form: str, b: int) -> np.ndarray:
    """The same by explicit loops over (c, h, w, i, j), one assignment per formula above: slow, for small tensors."""
    x = np.asarray(x)
    n, c, h, w = x.shape
    y = np.empty((n,) + out_shape(form, b, c, h, w), x.dtype)
    if form in TO_SPACE:
        cs = c // (b * b)
        for cc in range(cs):
            for hh in range(h):
                for ww in range(w):
                    for i in range(b):
                        for j in range(b):
                            src = (i * b + j) * cs + cc if form == "dcr" else cc * b * b + i * b + j
                            y[:, cc, hh * b + i, ww * b + j] = x[:, src, hh, ww]
    else:
        for cc in range(c):
            for hh in range(h // b):
                for ww in range(w // b):
                    for i in range(b):
                        for j in range(b):
                            dst = (i * b + j) * c + cc if form == "s2d" else cc * b * b + i * b + j
                            y[:, dst, hh, ww] = x[:, cc, hh * b + i, ww * b + j]
    return y


def flat_index_input(rows: int, shape) -> np.ndarray:
    """Every element holds its own flat index over the whole batch, which stays below 2^24 for the shapes the tests use (so it is exact in
    f32): a wrong source shows up as a value that names where it came from."""
    total = rows * int(np.prod(shape))
    assert total < (1 << 24), total
    return np.arange(total, dtype=np.float32).reshape((rows,) + tuple(shape))
