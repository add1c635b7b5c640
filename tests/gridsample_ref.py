"""GridSample and AffineGrid twice (INTEGRATION.md 2.6 "Grid sampling"): the contract's fixed sequence of separately rounded float32 operations
restated in numpy (float32 arrays round every operation once, as the kernel does), and the operator evaluated in float64 by torch on the CPU."""
from __future__ import annotations

import numpy as np

F = np.float32
MODES, PADDINGS, ALIGNS = ("bilinear", "nearest"), ("zeros", "border", "reflection"), (0, 1)


def pixel_coord(g, size, padding, align, clamp=True):
    """A normalised coordinate -> pixels of an axis of `size`, in g's own precision: un-normalise, reflect, clip (border, reflection), and with
    `clamp` the contract's clamp to [-2, size + 1] in front of the conversion to an integer.  -> (coordinate, was it NaN before or after the rule)"""
    T = g.dtype.type
    with np.errstate(invalid="ignore"):
        c = ((g + T(1)) * T(0.5)) * T(size - 1) if align else (((g + T(1)) * T(size)) - T(1)) * T(0.5)
        nan = np.isnan(c)
        if padding == "reflection":
            lo, span = (T(0), T(size - 1)) if align else (T(-0.5), T(size))
            d = np.abs(c - lo)
            c = np.where(np.fmod(np.floor(d / span), T(2)) == 0, np.fmod(d, span) + lo, (span - np.fmod(d, span)) + lo) if span else np.zeros_like(c)
            nan = nan | np.isnan(c)
        if padding != "zeros" and clamp:
            c = np.where(c >= 0, c, T(0))
            c = np.where(c <= T(size - 1), c, T(size - 1))
        if clamp:
            c = np.where(c >= T(-2), c, T(-2))
            c = np.where(c <= T(size + 1), c, T(size + 1))
    return c.astype(T), nan


def grid_sample32(x, grid, mode="bilinear", padding="zeros", align=0):
    """x [N,C,H,W], grid [N,Ho,Wo,2] -> [N,C,Ho,Wo], bit for bit what the kernel computes"""
    x, g = np.ascontiguousarray(x, F), np.asarray(grid, F)
    N, C, H, W = x.shape
    (ix, nx), (iy, ny) = pixel_coord(g[..., 0], W, padding, align), pixel_coord(g[..., 1], H, padding, align)
    n = np.arange(N)[:, None, None]

    def tap(yi, xi):
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        return np.where(inside[..., None], x[n, :, np.where(inside, yi, 0), np.where(inside, xi, 0)], F(0)).astype(F)  # [N,Ho,Wo,C]

    if mode == "nearest":
        y = tap(np.rint(iy).astype(np.int64), np.rint(ix).astype(np.int64))
    else:
        fx, fy = np.floor(ix), np.floor(iy)
        wx, wy = (F(1) - (ix - fx), ix - fx), (F(1) - (iy - fy), iy - fy)
        with np.errstate(invalid="ignore", over="ignore"):
            p = [tap(fy.astype(np.int64) + dy, fx.astype(np.int64) + dx) * (wy[dy] * wx[dx])[..., None] for dy in (0, 1) for dx in (0, 1)]
            y = ((p[0] + p[1]) + p[2]) + p[3]
    return np.ascontiguousarray(np.where((nx | ny)[..., None], F(np.nan), y).astype(F).transpose(0, 3, 1, 2))


def affine_grid32(theta, out_hw, align=0):
    """theta [N,6] -> the grid [N,Ho,Wo,2], bit for bit"""
    def base(size):
        j = np.arange(size)
        return ((2 * j).astype(F) / F(max(size - 1, 1)) - F(size > 1)).astype(F) if align else ((2 * j + 1).astype(F) / F(size) - F(1)).astype(F)

    t = np.asarray(theta, F).reshape(-1, 6)[:, None, None, :]
    xb, yb = base(out_hw[1])[None, None, :], base(out_hw[0])[None, :, None]
    return np.stack([((t[..., 0] * xb) + (t[..., 1] * yb)) + t[..., 2], ((t[..., 3] * xb) + (t[..., 4] * yb)) + t[..., 5]], axis=-1).astype(F)


def grid_sample64(x, grid, mode="bilinear", padding="zeros", align=0):
    import torch

    return torch.nn.functional.grid_sample(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(grid, np.float64)), mode=mode,
                                           padding_mode=padding, align_corners=bool(align)).numpy()


def tie_distance(grid, hw, mode, padding, align):
    """How far each coordinate (float64) is from where the result jumps: an integer (bilinear: floor) or a half (nearest: the pick).  A
    coordinate the padding rule clips counts by its distance from the clip's range: beyond it both precisions land on the same pixel."""
    d = []
    for k, size in ((0, hw[1]), (1, hw[0])):
        c = pixel_coord(np.asarray(grid, np.float64)[..., k], size, padding, align, clamp=False)[0]
        s = c + (0.5 if mode == "nearest" else 0.0)
        near = np.abs(s - np.rint(s))
        d.append(near if padding == "zeros" else np.where(c < 0, -c, np.where(c > size - 1, c - (size - 1), near)))
    return np.minimum(d[0], d[1])


def lattice_grid(n, out_hw, hw, align, lo=-1.5, hi=1.5):
    """A grid over [lo, hi]^2 whose pixel coordinates are odd multiples of 1/8 plus 1/32: 1/32 or more from every integer and every half, inside
    the image and, reflected, outside it.  Rows and images are permuted copies of one lattice."""
    size = np.array([hw[1], hw[0]], np.float64)
    m = int(np.prod(out_hw)) * n
    k = np.stack([np.linspace(lo, hi, m), np.linspace(hi, lo, m)[np.random.default_rng(m).permutation(m)]], axis=-1)
    c = (k + 1) / 2 * (size - 1) if align else ((k + 1) * size - 1) / 2
    c = np.floor(c * 4) / 4 + 0.125 + 1 / 32
    g = c / (size - 1) * 2 - 1 if align else (2 * c + 1) / size - 1
    return g.reshape((n,) + tuple(out_hw) + (2,)).astype(F)


def bound(hw, x, u=2.0 ** -24):
    """u (1 + max(H, W)) max|X|: a coordinate error of u W meets a slope of at most 2 max|X|; the measured margin multiplies it (profiles/gridsample_error_ratios.txt)"""
    return u * (1 + max(hw)) * float(np.abs(x).max())
