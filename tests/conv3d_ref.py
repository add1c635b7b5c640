"""Float64 restatement of Conv, MaxPool and AveragePool on [N, C, D, H, W] for tests/test_conv3d_gpu.py: pad, then one slice and one einsum per tap."""
from __future__ import annotations

import itertools

import numpy as np


def _taps(x, k, strides, pads, dilations, fill, out=None):
    """x padded with `fill`, and per tap (kz, ky, kx) the strided slice [N, C, OD, OH, OW] of it that the tap reads"""
    xp = np.pad(x.astype(np.float64), [(0, 0), (0, 0)] + [(pads[i], pads[i + 3]) for i in range(3)], constant_values=fill)
    out = out or [(xp.shape[2 + i] - dilations[i] * (k[i] - 1) - 1) // strides[i] + 1 for i in range(3)]
    for t in itertools.product(*(range(e) for e in k)):
        yield t, xp[(slice(None), slice(None)) + tuple(slice(t[i] * dilations[i], t[i] * dilations[i] + (out[i] - 1) * strides[i] + 1, strides[i]) for i in range(3))]


def conv3d(x, w, b=None, strides=(1, 1, 1), pads=(0,) * 6, dilations=(1, 1, 1), group=1):
    """(y, mag): the convolution in float64 and, per output element, sum |x| |w| + |b| over its taps (what the f32 error bound scales with)"""
    w = w.astype(np.float64)
    mg = w.shape[0] // group
    y = mag = 0.0
    for (kz, ky, kx), xs in _taps(x, w.shape[2:], strides, pads, dilations, 0.0):
        xg = xs.reshape(xs.shape[0], group, -1, *xs.shape[2:])
        wg = w[:, :, kz, ky, kx].reshape(group, mg, -1)
        y = y + np.einsum("ngcdhw,gmc->ngmdhw", xg, wg)
        mag = mag + np.einsum("ngcdhw,gmc->ngmdhw", np.abs(xg), np.abs(wg))
    y, mag = (a.reshape(a.shape[0], -1, *a.shape[3:]) for a in (y, mag))
    bias = 0.0 if b is None else b.astype(np.float64).reshape(1, -1, 1, 1, 1)
    return y + bias, mag + np.abs(bias)


def pool3d(x, op, kernel_shape, strides=(1, 1, 1), pads=(0,) * 6, ceil_mode=0, count_include_pad=0):
    """MaxPool / AveragePool: taps outside the volume are ignored (the average divides by the taps inside it, or by all of them)"""
    out = []
    for i in range(3):
        num = x.shape[2 + i] + pads[i] + pads[i + 3] - kernel_shape[i]
        o = (-(-num // strides[i]) if ceil_mode else num // strides[i]) + 1
        out.append(o - 1 if ceil_mode and (o - 1) * strides[i] >= x.shape[2 + i] + pads[i] else o)
    grown = [pads[i + 3] + strides[i] for i in range(3)]  # (room for the last window of ceil_mode)
    taps = [xs for _, xs in _taps(x, kernel_shape, strides, list(pads[:3]) + grown, (1, 1, 1), np.nan, out)]
    if op == "MaxPool":
        return np.nanmax(taps, axis=0)
    inside = np.sum(~np.isnan(taps), axis=0)
    return np.nansum(taps, axis=0) / (len(taps) if count_include_pad else inside)


def r3d(ops, x):
    """the float64 forward of onnx_writer.r3d_net's operation list"""
    v = [x.astype(np.float64)]
    for o in ops:
        if o[0] == "conv":
            _, w, (sc, b, mu, var), stride, pad, relu, src = o
            y = conv3d(v[src], w, None, stride, pad * 2)[0]
            f = sc.astype(np.float64) / np.sqrt(var.astype(np.float64) + np.float64(np.float32(1e-5)))
            y = (y - mu.astype(np.float64).reshape(1, -1, 1, 1, 1)) * f.reshape(1, -1, 1, 1, 1) + b.astype(np.float64).reshape(1, -1, 1, 1, 1)
            v.append(np.maximum(y, 0) if relu else y)
        elif o[0] == "pool":
            v.append(pool3d(v[-1], "MaxPool", (3, 3, 3), (2, 2, 2), (1,) * 6))
        elif o[0] == "add":
            v.append(np.maximum(v[o[1]] + v[o[2]], 0))
        else:
            return v[-1].mean(axis=(2, 3, 4)) @ o[1].astype(np.float64) + o[2].astype(np.float64)
