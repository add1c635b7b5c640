"""DeformConv in float64, a plain numpy loop straight from the coordinate contract (INTEGRATION.md 2.6 "Deformable convolutions"): the reference of
tests/test_deformconv_gpu.py.  Returns the result and, per output, the magnitude mag = sum |w| |mask| sum_corners weight |v| + |b| that the
error bound of the normal-valued run scales with."""
from __future__ import annotations

import numpy as np


def deform_conv64(x, w, off, b=None, mask=None, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1), group=1, offset_group=1):
    x, w, off = (np.asarray(a, np.float64) for a in (x, w, off))
    N, C, H, W = x.shape
    M, Cg, kh, kw = w.shape
    OH, OW = off.shape[2:]
    taps, Cog, Mg = kh * kw, C // offset_group, M // group
    mask = np.ones((N, offset_group * taps, OH, OW)) if mask is None else np.asarray(mask, np.float64)
    col = np.zeros((N, C, taps, OH, OW))   # the sampled, modulated column
    cabs = np.zeros_like(col)              # ... of |x|, under |mask|
    oh, ow = np.meshgrid(np.arange(OH), np.arange(OW), indexing="ij")
    for g in range(offset_group):
        for t in range(taps):
            i, j = divmod(t, kw)
            cy = (oh * strides[0] - pads[0] + i * dilations[0]) + off[:, (g * taps + t) * 2]
            cx = (ow * strides[1] - pads[1] + j * dilations[1]) + off[:, (g * taps + t) * 2 + 1]
            nan = np.isnan(cy) | np.isnan(cx)
            cy, cx = np.clip(np.where(nan, -2, cy), -2, H + 1), np.clip(np.where(nan, -2, cx), -2, W + 1)
            fy, fx = np.floor(cy), np.floor(cx)
            ty, tx = cy - fy, cx - fx
            v, va = np.zeros((N, Cog, OH, OW)), np.zeros((N, Cog, OH, OW))
            for dy, wy in ((0, 1 - ty), (1, ty)):
                for dx, wx in ((0, 1 - tx), (1, tx)):
                    y, xx = (fy + dy).astype(np.int64), (fx + dx).astype(np.int64)
                    inside = (y >= 0) & (y < H) & (xx >= 0) & (xx < W)
                    px = x[np.arange(N)[:, None, None, None], np.arange(g * Cog, (g + 1) * Cog)[None, :, None, None], np.clip(y, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[:, None]]
                    px = np.where(inside[:, None], px, 0.0)
                    v, va = v + px * (wy * wx)[:, None], va + np.abs(px) * (wy * wx)[:, None]
            mk = mask[:, g * taps + t][:, None]
            col[:, g * Cog:(g + 1) * Cog, t] = np.where(nan[:, None], np.nan, v * mk)
            cabs[:, g * Cog:(g + 1) * Cog, t] = np.where(nan[:, None], 0.0, va * np.abs(mk))
    y, mag = np.zeros((N, M, OH, OW)), np.zeros((N, M, OH, OW))
    for gi in range(group):
        wg = w[gi * Mg:(gi + 1) * Mg].reshape(Mg, Cg * taps)
        y[:, gi * Mg:(gi + 1) * Mg] = np.einsum("mk,nkhw->nmhw", wg, col[:, gi * Cg:(gi + 1) * Cg].reshape(N, Cg * taps, OH, OW))
        mag[:, gi * Mg:(gi + 1) * Mg] = np.einsum("mk,nkhw->nmhw", np.abs(wg), cabs[:, gi * Cg:(gi + 1) * Cg].reshape(N, Cg * taps, OH, OW))
    if b is not None:
        y, mag = y + np.asarray(b, np.float64)[None, :, None, None], mag + np.abs(np.asarray(b, np.float64))[None, :, None, None]
    return y, mag


def dcn_block64(w: dict, x, k: int, offset_group: int = 1):
    """onnx_writer.dcn_block's scores in float64"""
    import torch
    import torch.nn.functional as F

    t = {n: torch.from_numpy(np.asarray(v, np.float64)) for n, v in w.items()}
    lo = (k - 1) // 2
    pad = lambda a: F.pad(a, (lo, k - 1 - lo, lo, k - 1 - lo))
    s = F.relu(F.conv2d(torch.from_numpy(np.asarray(x, np.float64)), t["stem_w"], t["stem_b"], padding=1))
    off, mask = F.conv2d(pad(s), t["off_w"], t["off_b"]), torch.sigmoid(F.conv2d(pad(s), t["mask_w"], t["mask_b"]))
    d, _ = deform_conv64(s.numpy(), w["dcn_w"], off.numpy(), w["dcn_b"], mask.numpy(), pads=(lo, lo, k - 1 - lo, k - 1 - lo), offset_group=offset_group)
    return F.conv2d(F.relu(torch.from_numpy(d)), t["head_w"], t["head_b"]).mean((2, 3)).numpy()
