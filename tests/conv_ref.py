"""A float64 restatement of the channel-quad convolution side (hip/conv.hip, conv_split.hip: tiled, weight-stationary, patch / stem, stem + pool,
bf16x6 split, depthwise, pools, global pools, concat / slice / shuffle), from numpy alone, the two probes that let a test read a channel-quad
feature map element by element, the inputs on which a correct kernel has exactly one right f32 answer, and the bound every other input is held
to.  A helper module (tests/test_conv_ref.py checks it without a GPU, tests/test_conv_exact_gpu.py uses it on one), not a conftest.

A case is {"id", "inp": (C0, H, W), "ops": [...], "env": {...}, "expect": [exec kinds], "kinds": (...), "rows": (...)}; an op is a dict
{"op": "conv" | "maxpool" | "avgpool" | "gap" | "gmp" | "concat" | "slice" | "shuffle" | "lrn" | "gate" | "bn", ...}; tensor 0 is the caller's NCHW
input, tensor i the result of op i - 1; "src" names what an op reads (default: the previous tensor), "add" the tensor a convolution's residual Add
takes, "gate" the [C, 1, 1] tensor a gate multiplies its "src" by.  A case may name the probe it is served through ("probe", default "A") and the
layout its plan must have ("layout", default "NC/4HW4"): probe "" serves the tensor itself, which keeps the plan in NCHW on conv2d_generic_kernel,
pool2d_kernel and the NCHW branches of the element-wise kernels (GENERIC_NCHW, NEIGHBOURS_NCHW, and the second run of every PER_CHANNEL case).

The probes.  A served [C, H, W] tensor forces the whole plan to NCHW and the generic kernel (schedule.cpp decide_layout), so the fast kernels were
only ever seen through a GlobalAveragePool -- which divides a wrong border pixel by H W before anyone compares.  Probe A ends the graph in a
ConvTranspose with a 1x1, stride-1, identity C x C weight: the transposed convolution stores NCHW itself (the plan stays NC/4HW4) and
1 * x + 0 * ... is exact for finite data.  Probe B ends it in Flatten -> MatMul with a one-hot K x n matrix: n chosen elements, exactly, through
the weight-row permutation of decide_layout.

Exact data.  "grid": integer inputs, weights (|w| <= 8: one bf16 part) and biases, every partial sum of every layer below 2^24 -- any order of
additions gives the same f32.  "select": every output feature has ONE nonzero weight +-2^e at one (channel, tap), activations are full-mantissa
f32 (dense_ref.full_mantissa): the result is +-2^e x to the bit, so a dropped low bit or a wrong tap / channel / pixel shows.  "onehot": at most
one nonzero activation (1.0) in each receptive field, full-mantissa weights: the result is the weight to the bit.

Exact on bf16x6 too (conv_split.hip).  cut3 (host, weights) and split3_pair (device, activations) cut v = hi + mid + lo by truncation, each part a
bf16, the subtractions exact; the kernel keeps hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi and drops mid*lo, lo*mid, lo*lo -- every dropped
product has a non-hi part on BOTH sides.  A weight that is one bf16 (grid: |w| <= 8; select: +-2^e) has mid = lo = 0: x_hi w, x_mid w, x_lo w are
all kept, each exact in f32 (8 x 8 bits), and their sum smallest first is x w.  The set is symmetric, so an activation that is one bf16 (onehot:
1.0) keeps w_hi, w_mid, w_lo the same way: onehot IS exact there and stays in.

The bound (error_bound).  A convolution's f32 sum of K = (C / groups) kh kw products, in ANY order, rounds each product and each partial sum once,
each within 2^-24 of a partial result that never exceeds mag = |x| * |w| + |b| (the same convolution of absolute values); with the bias, the residual
add and the final rounding that is (K + 3) 2^-24 mag.  The error e of the layer's input arrives through |w|:

    e_l = (K_l + 3) 2^-24 mag_l + |w_l| * e_(l-1) + e_residual,       mag_l = (|h_(l-1)| + e_(l-1)) * |w_l| + |b_l| + |residual|.

bf16x6: six partial products per term, each exact, each added to the f32 accumulator: (6 K + 3) 2^-24 mag; and the three dropped products.  hi keeps
8 significant bits, so |mid| <= |v - hi| < 2^-7 |v|, and |lo| < 2^-7 |v - hi| < 2^-14 |v|: |x_mid w_lo| + |x_lo w_mid| + |x_lo w_lo| <
(2^-21 + 2^-21 + 2^-28) |x| |w| < 2^-19.99 |x w|, summed over the terms: (2^-20 + 2^-28) mag.  Activations: Relu, Clip, LeakyRelu 1-Lipschitz (LeakyRelu
one more rounding), Sigmoid (1/4) and Tanh 2 ulp of the value (device_common.hpp).  Max pools pass the largest error of the window on, average pools
the mean plus (n + 1) roundings of the window's |x| sum.  The generic kernel's chain is one MFMA fma per term: the same (K + 3) 2^-24 mag.

Per-channel operators.  gate y = x g: |g| e_x + |x| e_g + U |x g| (one product).  bn y = s x + t (fused or not): |s| e_x + 2 U (|s x| + |t|).
lrn y = x / (bias + alpha / size * sum v^2)^beta: the window sum is `size` fmas, (size + 1) U sum v^2, plus 2 |v| e_v from the input, carried to y
through d y / d sum; powf and the division have no accuracy figure in device_common.hpp or in the ROCm documents, so LRN's generic data is held
to the project's parity bar |got - ref| <= 1e-4 |ref| + 1e-6 against float64 (lrn_bar) and that bar is what forward64 adds for them.  Its exact
checks need none: alpha = 0, bias = 1 gives pow(1, beta) == 1 and y == x to the bit (lrn_identity), and the two layouts give the same bits."""
from __future__ import annotations

import math

import numpy as np

from infera_amd import onnx_writer as W
from tests.dense_ref import full_mantissa, rms  # noqa: F401  (rms: re-exported for the GPU tests)

U = 2.0 ** -24
LEAKY = np.float32(0.25)  # a power of two: exact on a grid
CLIP = (np.float32(-3.0), np.float32(6.0))
ACTS = ("Relu", "Sigmoid", "Tanh", "LeakyRelu", "Clip")  # what the MFMA epilogues fuse (plan.hpp kMaxMfmaFusedAct)
CUS = 256  # compute units of an MI355X: mt_pick and the persistent grid of the weight-stationary kernel depend on it


# ---- float64 operators ------------------------------------------------------------------------------------------------------------

def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _pads(p):
    return (p,) * 4 if isinstance(p, int) else tuple(p)  # ONNX order: top, left, bottom, right


def out_hw(hw, k, s=1, p=0, d=1, ceil_mode=False):
    k, s, d, p = _pair(k), _pair(s), _pair(d), _pads(p)
    out = []
    for a in range(2):
        span = hw[a] + p[a] + p[a + 2] - ((k[a] - 1) * d[a] + 1)
        o = (-(-span // s[a]) if ceil_mode else span // s[a]) + 1
        if ceil_mode and (o - 1) * s[a] >= hw[a] + p[a]:  # a window that starts past the input and its leading pad is dropped
            o -= 1
        out.append(o)
    return tuple(out)


def in_hw(ohw, k, s=1, p=0, d=1):
    """the smallest input extent whose convolution has `ohw` outputs"""
    k, s, d, p = _pair(k), _pair(s), _pair(d), _pads(p)
    return tuple((ohw[a] - 1) * s[a] + (k[a] - 1) * d[a] + 1 - p[a] - p[a + 2] for a in range(2))


def conv2d64(x, w, b=None, s=1, p=0, d=1, groups=1):
    """x [N, C, H, W], w [M, C / groups, kh, kw] -> [N, M, OH, OW] in float64"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    s, d, p = _pair(s), _pair(d), _pads(p)
    N, C, H, Wd = x.shape
    M, Cg, kh, kw = w.shape
    assert C == Cg * groups and M % groups == 0
    OH, OW = out_hw((H, Wd), (kh, kw), s, p, d)
    xp = np.zeros((N, C, H + p[0] + p[2], Wd + p[1] + p[3]))
    xp[:, :, p[0]:p[0] + H, p[1]:p[1] + Wd] = x
    y = np.zeros((N, M, OH, OW))
    Mg = M // groups
    for g in range(groups):
        for ky in range(kh):
            for kx in range(kw):
                win = xp[:, g * Cg:(g + 1) * Cg, ky * d[0]:ky * d[0] + (OH - 1) * s[0] + 1:s[0], kx * d[1]:kx * d[1] + (OW - 1) * s[1] + 1:s[1]]
                y[:, g * Mg:(g + 1) * Mg] += np.einsum("nchw,mc->nmhw", win, w[g * Mg:(g + 1) * Mg, :, ky, kx])
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None, None]
    return y


def pool64(x, kind, k, s=1, p=0, d=1, ceil_mode=False, count_include_pad=False, parts=False):
    """MaxPool / AveragePool (ONNX): windows clipped to the input (max; average without count_include_pad) or to the padded extent; `parts`: the
    window sums and the divisors of an average pool instead of their quotient"""
    x = np.asarray(x, np.float64)
    k, s, d, p = _pair(k), _pair(s), _pair(d), _pads(p)
    N, C, H, Wd = x.shape
    OH, OW = out_hw((H, Wd), k, s, p, d, ceil_mode)
    y = np.full((N, C, OH, OW), -np.inf if kind == "max" else 0.0)
    cnt = np.ones((OH, OW))
    for oy in range(OH):
        for ox in range(OW):
            ys = [oy * s[0] - p[0] + i * d[0] for i in range(k[0])]
            xs = [ox * s[1] - p[1] + j * d[1] for j in range(k[1])]
            yin, xin = [v for v in ys if 0 <= v < H], [v for v in xs if 0 <= v < Wd]
            if not yin or not xin:
                continue
            win = x[:, :, yin][:, :, :, xin]
            if kind == "max":
                y[:, :, oy, ox] = win.max(axis=(2, 3))
            else:
                n = len(yin) * len(xin)
                if count_include_pad:
                    n = len([v for v in ys if -p[0] <= v < H + p[2]]) * len([v for v in xs if -p[1] <= v < Wd + p[3]])
                y[:, :, oy, ox] = win.sum(axis=(2, 3))
                cnt[oy, ox] = n
    if kind == "max":
        return y
    return (y, cnt) if parts else y / cnt


def act64(z, kind):
    if kind == "Relu":
        return np.maximum(z, 0.0)
    if kind == "Sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    if kind == "Tanh":
        return np.tanh(z)
    if kind == "LeakyRelu":
        return np.where(z >= 0, z, np.float64(LEAKY) * z)
    if kind == "Clip":
        return np.clip(z, float(CLIP[0]), float(CLIP[1]))
    assert kind == "", kind
    return z


def shuffle64(x, groups):
    n, c, h, w = x.shape
    return x.reshape(n, groups, c // groups, h, w).transpose(0, 2, 1, 3, 4).reshape(n, c, h, w)


def lrn64(x, size, alpha, beta, bias, parts=False):
    """ONNX LRN over the channel axis: the window [c - (size - 1) // 2, c + size - 1 - (size - 1) // 2] clipped to the channels, alpha / size of
    its sum of squares whatever the clipping; `parts`: (the window sums of squares, bias + alpha / size * them) as well"""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    lo = (size - 1) // 2
    hi = size - 1 - lo
    sq = np.stack([(x[:, max(c - lo, 0):min(c + hi, C - 1) + 1] ** 2).sum(1) for c in range(C)], 1)
    base = bias + alpha / size * sq
    y = x / base ** beta
    return (y, sq, base) if parts else y


def lrn_bar(ref):
    """the project's parity bar, for what powf and the division add (module docstring)"""
    return 1e-4 * np.abs(ref) + 1e-6


# ---- ops, shapes, reference, bound --------------------------------------------------------------------------------------------------

def conv(M, k=1, s=1, p=0, d=1, g=1, bias=True, act="", add=None, src=None):
    return {"op": "conv", "M": M, "k": _pair(k), "s": _pair(s), "p": _pads(p), "d": _pair(d), "g": g, "bias": bias, "act": act, "add": add, "src": src}


def pool(kind, k, s=1, p=0, d=1, ceil=False, cip=False, src=None):
    return {"op": kind + "pool", "k": _pair(k), "s": _pair(s), "p": _pads(p), "d": _pair(d), "ceil": ceil, "cip": cip, "src": src}


def lrn(size, alpha=1e-4, beta=0.75, bias=1.0, src=None):
    f = lambda v: float(np.float32(v))  # (the attributes are f32)
    return {"op": "lrn", "size": size, "alpha": f(alpha), "beta": f(beta), "bias": f(bias), "src": src}


def gate(src, gate):
    """tensor `src` [C, H, W] times tensor `gate` [C, 1, 1] (squeeze and excitation)"""
    return {"op": "gate", "src": src, "gate": gate}


def bn(src=None):
    """a BatchNormalization with mean 0, variance 1 and epsilon 0: y = scale x + shift with (scale, shift) = weights[op index], as they are"""
    return {"op": "bn", "src": src}


def shapes(case):
    """the (C, H, W) of every tensor of the case, tensor 0 being the input"""
    sh = [tuple(case["inp"])]
    for i, o in enumerate(case["ops"]):
        c, h, w = sh[o["src"] if o.get("src") is not None else i]
        if o["op"] == "conv":
            sh.append((o["M"], *out_hw((h, w), o["k"], o["s"], o["p"], o["d"])))
        elif o["op"] in ("maxpool", "avgpool"):
            sh.append((c, *out_hw((h, w), o["k"], o["s"], o["p"], o["d"], o["ceil"])))
        elif o["op"] in ("gap", "gmp"):
            sh.append((c, 1, 1))
        elif o["op"] == "concat":
            sh.append((sum(sh[t][0] for t in o["srcs"]), *sh[o["srcs"][0]][1:]))
        elif o["op"] == "slice":
            sh.append((o["c1"] - o["c0"], h, w))
        else:
            assert o["op"] in ("shuffle", "lrn", "gate", "bn"), o
            sh.append((c, h, w))
    return sh


def forward64(case, weights, x, bound: bool = False, split=()):
    """the float64 value of every tensor ([rows, C, H, W]); with `bound` also the per-element error bound of the module docstring, the convolutions
    whose op index is in `split` held to the bf16x6 term"""
    t = [np.asarray(x, np.float64).reshape(-1, *case["inp"])]
    e = [np.zeros_like(t[0])]
    mags = []
    for i, o in enumerate(case["ops"]):
        src = o["src"] if o.get("src") is not None else i
        h, eh = t[src], e[src]
        if o["op"] == "conv":
            w, b = weights[i]
            geo = dict(s=o["s"], p=o["p"], d=o["d"], groups=o["g"])
            z = conv2d64(h, w, b, **geo)
            res = t[o["add"]] if o["add"] is not None else None
            if res is not None:
                z = z + res
            y = act64(z, o["act"])
            K = w.shape[1] * w.shape[2] * w.shape[3]
            mag = conv2d64(np.abs(h) + eh, np.abs(w), None if b is None else np.abs(b), **geo) + (0 if res is None else np.abs(res))
            mags.append(mag)
            if bound:
                terms = (6 * K + 3) * U + (2.0 ** -20 + 2.0 ** -28) if i in split else (K + 3) * U
                ez = terms * mag + conv2d64(eh, np.abs(w), None, **geo) + (0 if res is None else e[o["add"]])
                if o["act"] == "Sigmoid":
                    ez = ez / 4 + 4 * U * np.abs(y)
                elif o["act"] == "Tanh":
                    ez = ez + 4 * U * np.abs(y)
                elif o["act"] == "LeakyRelu":
                    ez = ez + U * np.abs(y)
            else:
                ez = np.zeros_like(y)
        elif o["op"] in ("maxpool", "avgpool"):
            kind = o["op"][:3]
            y = pool64(h, kind, o["k"], o["s"], o["p"], o["d"], o["ceil"], o["cip"])
            if kind == "max":
                ez = np.maximum(pool64(eh, "max", o["k"], o["s"], o["p"], o["d"], o["ceil"]), 0.0)
            else:
                n = o["k"][0] * o["k"][1]
                ez = pool64(eh, "avg", o["k"], o["s"], o["p"], o["d"], o["ceil"], o["cip"]) + (n + 1) * U * pool64(np.abs(h), "avg", o["k"], o["s"], o["p"], o["d"], o["ceil"], o["cip"])
        elif o["op"] == "gap":
            y = h.mean(axis=(2, 3), keepdims=True)
            n = h.shape[2] * h.shape[3]
            ez = eh.mean(axis=(2, 3), keepdims=True) + (n + 1) * U * np.abs(h).mean(axis=(2, 3), keepdims=True)
        elif o["op"] == "gmp":
            y, ez = h.max(axis=(2, 3), keepdims=True), eh.max(axis=(2, 3), keepdims=True)
        elif o["op"] == "concat":
            y, ez = np.concatenate([t[s] for s in o["srcs"]], 1), np.concatenate([e[s] for s in o["srcs"]], 1)
        elif o["op"] == "slice":
            y, ez = h[:, o["c0"]:o["c1"]], eh[:, o["c0"]:o["c1"]]
        elif o["op"] == "shuffle":
            y, ez = shuffle64(h, o["groups"]), shuffle64(eh, o["groups"])
        elif o["op"] == "gate":
            g, eg = t[o["gate"]], e[o["gate"]]
            y = h * g
            ez = np.abs(g) * eh + np.abs(h) * eg + U * np.abs(y)
        elif o["op"] == "bn":
            sc, sf = (np.asarray(v, np.float64)[None, :, None, None] for v in weights[i])
            y = sc * h + sf
            ez = np.abs(sc) * eh + 2 * U * (np.abs(sc * h) + np.abs(sf))
        else:
            assert o["op"] == "lrn", o
            y, sq, base = lrn64(h, o["size"], o["alpha"], o["beta"], o["bias"], parts=True)
            _, cross, _ = lrn64(np.sqrt(np.abs(h) * eh), o["size"], o["alpha"], o["beta"], o["bias"], parts=True)  # the window's sum of |v| e_v
            e_sq = (o["size"] + 1) * U * sq + 2 * cross
            ez = eh / base ** o["beta"] + np.abs(y) * o["beta"] * (o["alpha"] / o["size"]) * e_sq / base + lrn_bar(y)
        t.append(y)
        e.append(ez)
    return {"t": t, "out": t[-1], "e": e[-1], "mag": mags}


def split_ops(case, plan_exec=None):
    """the op indices of the convolutions the case expects on the bf16x6 kernels"""
    kinds = [k for k in case["expect"] or () if k != "convt_phase"]  # (no list: an NCHW plan, nothing on bf16x6)
    return {i for i, k in enumerate(kinds[:len(case["ops"])]) if k in ("conv_split_bf16x6", "conv_patch_pool_bf16x6")}


def error_bound(case, weights, x):
    """(the float64 reference of the feature map [rows, C, H, W], the bound on |served - reference| per element)"""
    r = forward64(case, weights, x, bound=True, split=split_ops(case))
    return r["out"], r["e"]


# ---- the graph ----------------------------------------------------------------------------------------------------------------------

def through_probe(ref, probe: str):
    """the f32 tensor `ref` as the probe hands it on: probe A's transposed convolution adds the other channels' 0 * x to 1 * x, so a -0.0 (a negative
    value times a gate of zero) leaves it as +0.0 and everything else to the bit; probe "" is the tensor itself, the sign of a zero included"""
    return ref + np.float32(0.0) if probe == "A" and ref.shape[-1] * ref.shape[-2] > 1 else ref


def probe_positions(shape, n: int = 48):
    """flat NCHW indices probe B reads: the four corners of the first and the last channel, then a stride through the tensor"""
    C, H, Wd = shape
    K = C * H * Wd
    idx = [(c * H + y) * Wd + x for c in (0, C - 1) for y in (0, H - 1) for x in (0, Wd - 1)]
    step = max(1, K // n) | 1
    idx += [(7 + step * i) % K for i in range(n)]
    return np.array(sorted(set(idx)), np.int64)


def graph(case, weights, probe: str = "A") -> bytes:
    """the case as an ONNX model with explicit weights, its last tensor served through probe A or B, as it is (probe ""), or, where it is [C, 1, 1], flattened"""
    sh = shapes(case)
    nodes, inits, names = [], [], ["X"]
    for i, o in enumerate(case["ops"]):
        src = names[o["src"] if o.get("src") is not None else i]
        out = f"t{i + 1}"
        if o["op"] == "conv":
            w, b = weights[i]
            inits.append(W.tensor(f"w{i}", np.ascontiguousarray(w, np.float32)))
            ins = [src, f"w{i}"]
            if b is not None:
                inits.append(W.tensor(f"b{i}", np.ascontiguousarray(b, np.float32)))
                ins.append(f"b{i}")
            attrs = [W.attr_ints("kernel_shape", o["k"]), W.attr_ints("strides", o["s"]), W.attr_ints("pads", o["p"]), W.attr_ints("dilations", o["d"]),
                     W.attr_i("group", o["g"])]
            cur = f"c{i}"
            nodes.append(W.node("Conv", ins, [cur], attrs))
            if o["add"] is not None:
                nodes.append(W.node("Add", [cur, names[o["add"]]], [f"a{i}"]))
                cur = f"a{i}"
            if o["act"] == "Clip":
                inits += [W.tensor(f"lo{i}", np.array(CLIP[0], np.float32)), W.tensor(f"hi{i}", np.array(CLIP[1], np.float32))]
                nodes.append(W.node("Clip", [cur, f"lo{i}", f"hi{i}"], [out]))
            elif o["act"]:
                nodes.append(W.node(o["act"], [cur], [out], [W.attr_f("alpha", float(LEAKY))] if o["act"] == "LeakyRelu" else []))
            else:
                nodes.append(W.node("Identity", [cur], [out]))
        elif o["op"] in ("maxpool", "avgpool"):
            attrs = [W.attr_ints("kernel_shape", o["k"]), W.attr_ints("strides", o["s"]), W.attr_ints("pads", o["p"]), W.attr_i("ceil_mode", int(o["ceil"]))]
            if o["op"] == "maxpool":
                attrs.append(W.attr_ints("dilations", o["d"]))
            else:
                assert o["d"] == (1, 1)
                attrs.append(W.attr_i("count_include_pad", int(o["cip"])))
            nodes.append(W.node("MaxPool" if o["op"] == "maxpool" else "AveragePool", [src], [out], attrs))
        elif o["op"] in ("gap", "gmp"):
            nodes.append(W.node("GlobalAveragePool" if o["op"] == "gap" else "GlobalMaxPool", [src], [out]))
        elif o["op"] == "concat":
            nodes.append(W.node("Concat", [names[s] for s in o["srcs"]], [out], [W.attr_i("axis", 1)]))
        elif o["op"] == "slice":
            inits += [W.tensor(f"s0_{i}", np.array([o["c0"]], np.int64)), W.tensor(f"s1_{i}", np.array([o["c1"]], np.int64)), W.tensor(f"sa_{i}", np.array([1], np.int64))]
            nodes.append(W.node("Slice", [src, f"s0_{i}", f"s1_{i}", f"sa_{i}"], [out]))
        elif o["op"] == "lrn":
            nodes.append(W.node("LRN", [src], [out], [W.attr_i("size", o["size"]), W.attr_f("alpha", o["alpha"]), W.attr_f("beta", o["beta"]), W.attr_f("bias", o["bias"])]))
        elif o["op"] == "gate":
            nodes.append(W.node("Mul", [src, names[o["gate"]]], [out]))
        elif o["op"] == "bn":
            sc, sf = (np.ascontiguousarray(v, np.float32) for v in weights[i])
            inits += [W.tensor(f"bs{i}", sc), W.tensor(f"bb{i}", sf), W.tensor(f"bm{i}", np.zeros_like(sc)), W.tensor(f"bv{i}", np.ones_like(sc))]
            nodes.append(W.node("BatchNormalization", [src, f"bs{i}", f"bb{i}", f"bm{i}", f"bv{i}"], [out], [W.attr_f("epsilon", 0.0)]))
        else:
            assert o["op"] == "shuffle", o
            c, h, w_ = sh[i + 1]
            inits += [W.tensor(f"r5_{i}", np.array([0, o["groups"], c // o["groups"], h, w_], np.int64)), W.tensor(f"r4_{i}", np.array([0, c, h, w_], np.int64))]
            nodes += [W.node("Reshape", [src, f"r5_{i}"], [f"p5_{i}"]), W.node("Transpose", [f"p5_{i}"], [f"q5_{i}"], [W.attr_ints("perm", [0, 2, 1, 3, 4])]),
                      W.node("Reshape", [f"q5_{i}", f"r4_{i}"], [out])]
        names.append(out)
    C, H, Wd = sh[-1]
    if H * Wd == 1:
        nodes.append(W.node("Flatten", [names[-1]], ["Y"], [W.attr_i("axis", 1)]))
        outs = [W.value_info("Y", ["N", C])]
    elif probe == "A":
        inits.append(W.tensor("probe_eye", np.eye(C, dtype=np.float32).reshape(C, C, 1, 1)))
        nodes.append(W.node("ConvTranspose", [names[-1], "probe_eye"], ["Y"], [W.attr_ints("kernel_shape", [1, 1]), W.attr_ints("strides", [1, 1])]))
        outs = [W.value_info("Y", ["N", C, H, Wd])]
    elif probe == "":  # the tensor itself: a [C, H, W] output keeps the plan NCHW -- for the oracle, which has no layouts (and no ConvTranspose)
        nodes.append(W.node("Identity", [names[-1]], ["Y"]))
        outs = [W.value_info("Y", ["N", C, H, Wd])]
    else:
        assert probe == "B", probe
        idx = probe_positions(sh[-1])
        sel = np.zeros((C * H * Wd, len(idx)), np.float32)
        sel[idx, np.arange(len(idx))] = 1.0
        inits.append(W.tensor("probe_sel", sel))
        nodes += [W.node("Flatten", [names[-1]], ["flat"], [W.attr_i("axis", 1)]), W.node("MatMul", ["flat", "probe_sel"], ["Y"])]
        outs = [W.value_info("Y", ["N", len(idx)])]
    return W.model("conv_ref", nodes, inits, [W.value_info("X", ["N", *case["inp"]])], outs)


# ---- inputs with one right answer ---------------------------------------------------------------------------------------------------

def _selection_conv(rng, M, Cg, k, groups, m0_phase=0):
    """every output feature: one +-2^e at one (channel, tap); the tap cycles with the feature, the channel strides through the group so that a layer
    with fewer features than channels still reads every 8-channel block"""
    kh, kw = k
    nt = kh * kw
    w = np.zeros((M, Cg, kh, kw), np.float32)
    a = next(s for s in range(max(1, -(-Cg // max(1, M // groups))), 2 * Cg + 2) if math.gcd(s, Cg) == 1)
    for m in range(M):
        tap, c = (m + m // nt + m0_phase) % nt, (a * m + Cg - 1 - a * (M - 1)) % Cg  # the last feature reads the last channel
        w[m, c, tap // kw, tap % kw] = np.ldexp(rng.choice([-1.0, 1.0]), int(rng.integers(-3, 4)))
    return w


def onehot_stem(C):
    """the 1x1 stem of an onehot case, 8 -> C channels: input channels 0..6 carry the bits of a channel number, channel 7 a 'lit' flag; feature m =
    Relu(lit + sum_j (+1 if bit j of m else -1) x_j - popcount(m)) is 1 where the pixel is lit with m's number and 0 elsewhere -- all integers"""
    assert C <= 128
    m = np.arange(C)
    bits = (m[:, None] >> np.arange(7)[None, :]) & 1
    w = np.concatenate([np.where(bits == 1, 1.0, -1.0), np.ones((C, 1))], 1).astype(np.float32).reshape(C, 8, 1, 1)
    return w, (-bits.sum(1)).astype(np.float32)


def _lattice(shape_hw, o, rows, channels, rng_phase=0):
    """(row, y, x, channel) of the lit pixels: a lattice whose period is the filter's span, so every receptive field holds at most one of them (and the
    padding the rest); the lattice's offset moves with the row, the channel with the pixel: every tap and every channel meets every kind of pixel"""
    H, Wd = shape_hw
    py, px = (o["k"][0] - 1) * o["d"][0] + 1, (o["k"][1] - 1) * o["d"][1] + 1
    out, n = [], rng_phase
    for r in range(rows):
        for y in range((r * 2 + 1) % py, H, py):
            for x in range((r + 1) % px, Wd, px):
                out.append((r, y, x, (5 * n + 3 * r) % channels))
                n += 1
    return out


def exact_case(case, kind: str, rows: int, seed: int = 0):
    """(weights {op index: (w, b)}, x [rows, C0 H W]) of kind "grid", "select" or "onehot"; the convolutions keep the case's geometry, activations
    and residual adds (select / onehot: no bias -- a sum of two values has a rounding; onehot: the first convolution is onehot_stem unless the
    case's only convolution is the stem itself)"""
    rng = np.random.default_rng([seed, {"grid": 1, "select": 2, "onehot": 3}[kind], *case["inp"], len(case["ops"])])
    sh = shapes(case)
    C0, H, Wd = case["inp"]
    weights = {}
    convs = [i for i, o in enumerate(case["ops"]) if o["op"] == "conv"]
    for i, o in enumerate(case["ops"]):
        if o["op"] == "bn":  # powers of two and small integers: exact on a grid
            assert kind == "grid", "s x + t has a rounding"
            c = sh[i + 1][0]
            weights[i] = (np.resize(np.array([2, -1, 0.5, 3, -4, 1, -0.25, 5], np.float32), c), ((np.arange(c) * 5) % 11 - 5).astype(np.float32))
    for n, i in enumerate(convs):
        o = case["ops"][i]
        Cin = sh[o["src"] if o.get("src") is not None else i][0]
        Cg = Cin // o["g"]
        if kind == "grid":
            lim = 2 if n == 0 and len(convs) > 1 else 8
            w = rng.integers(-lim, lim + 1, (o["M"], Cg, *o["k"])).astype(np.float32)
            b = rng.integers(-8, 9, o["M"]).astype(np.float32) if o["bias"] else None
        elif kind == "select":
            assert o["add"] is None and o["act"] in ("", "Relu"), "a selection has no residual and no rounding activation"
            w, b = _selection_conv(rng, o["M"], Cg, o["k"], o["g"]), None
        else:
            assert o["add"] is None and o["act"] in ("", "Relu")
            if n == 0 and len(convs) > 1:
                assert o["k"] == (1, 1) and Cin == 8 and o["act"] == "Relu" and o["bias"], "an onehot case starts with the 8 -> C one-hot stem"
                w, b = onehot_stem(o["M"])
            else:
                w, b = full_mantissa(rng, (o["M"], Cg, *o["k"])), None
        weights[i] = (w, b)
    if kind == "grid":
        x = rng.integers(-4, 5, (rows, C0 * H * Wd)).astype(np.float32)
    elif kind == "select":
        x = full_mantissa(rng, (rows, C0 * H * Wd))
    else:
        x = np.zeros((rows, C0, H, Wd), np.float32)
        last = case["ops"][convs[-1]]
        if len(convs) > 1:
            assert convs[:2] == [0, 1] and len(convs) == 2, "stem, then the convolution under test"
            for r, y, xx, c in _lattice((H, Wd), last, rows, sh[1][0]):
                x[r, :7, y, xx] = (c >> np.arange(7)) & 1
                x[r, 7, y, xx] = 1.0
        else:
            g, Cg = last["g"], C0 // last["g"]  # one lit channel in EVERY group: each receptive field holds at most one activation per group
            for n, (r, y, xx, c) in enumerate(_lattice((H, Wd), last, rows, Cg)):
                for grp in range(g):
                    x[r, grp * Cg + (c + grp) % Cg, y, xx] = np.ldexp(1.0, (n + grp) % 7 - 3)
        x = x.reshape(rows, -1)
    return weights, x


def assert_exact(case, weights, x, kind: str):
    """the case has ONE right f32 answer whatever the summation order: every convolution's float64 sums and every tensor ARE f32 values (grid: and
    every partial sum an integer below 2^24; select / onehot: every output is one product or zero); returns the reference as f32 [rows, C, H, W]"""
    r = forward64(case, weights, x)
    for t in r["t"]:
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t), "a tensor of the reference is no f32 value"
    convs = [i for i, o in enumerate(case["ops"]) if o["op"] == "conv"]
    if kind == "grid":
        # (behind a global average pool of 2^j pixels the values are integers / 2^j: the partial sums stay exact below 2^24 / 2^j)
        px = [int(np.prod(r["t"][o["src"] if o.get("src") is not None else j].shape[2:])) if o["op"] == "gap" else 1 for j, o in enumerate(case["ops"])]
        denom = [int(np.prod(px[:i])) for i in convs]
        assert all(d & (d - 1) == 0 and m.max() * d < 2 ** 24 for d, m in zip(denom, r["mag"])), [m.max() for m in r["mag"]]
        for i, o in enumerate(case["ops"]):
            if o["op"] in ("gate", "bn"):  # one product (and one sum) of such values: an f32 value (checked above) with nothing rounded before it
                assert np.abs(r["t"][i + 1]).max() * max(denom) < 2 ** 24
        for i in convs:
            w, b = weights[i]
            assert np.array_equal(w, np.round(w)) and np.abs(w).max() <= 8 and (b is None or np.array_equal(b, np.round(b)))
        assert not any(o.get("act") in ("Sigmoid", "Tanh") for o in case["ops"]) and not any(o["op"] == "avgpool" for o in case["ops"])
    else:
        for n, i in enumerate(convs):
            o = case["ops"][i]
            w, _ = weights[i]
            if kind == "onehot" and n == 0 and len(convs) > 1:
                continue  # (the integer stem: checked by its output being one-hot below)
            src = r["t"][o["src"] if o.get("src") is not None else i]
            if kind == "select":
                assert (np.count_nonzero(w.reshape(w.shape[0], -1), axis=1) == 1).all()
                nz = np.abs(w[w != 0])
                assert np.array_equal(np.log2(nz), np.round(np.log2(nz)))
            else:
                ones = conv2d64((src != 0).astype(np.float64), np.ones((o["g"], src.shape[1] // o["g"], *o["k"])), None, o["s"], o["p"], o["d"], o["g"])
                assert ones.max() <= 1, "two lit activations in one receptive field of one group"
                nz = src[src != 0]
                assert np.array_equal(np.log2(np.abs(nz)), np.round(np.log2(np.abs(nz))))  # one bf16 part each
    return r["out"].astype(np.float32)


# ---- which kernel serves a layer (conv.hip / conv_split.hip, restated) ---------------------------------------------------------------

def tiled_supported(C, M, k, groups=1):
    return groups == 1 and C % 4 == 0 and M % 4 == 0 and k[0] * k[1] <= 64


def padc(C, M) -> bool:
    """conv2d_tiled_geom: channel counts that are no multiples of 32 run zero-padded to 32 (MODE 2)"""
    return not (C % 32 == 0 and M % 32 == 0)


def mt_pick(C, M, k, s, total_pix, cus: int = CUS) -> int:
    """conv2d_tiled: feature tiles per workgroup -- the largest of 4, 3, 2, 1 that divides M / 32; a stride-1 filter of more than one tap falls from 4 to
    2 while the launch has fewer than 8 rounds of workgroups"""
    pad = padc(C, M)
    m32 = (M + 31) // 32
    mt = 4 if m32 % 4 == 0 else 3 if m32 % 3 == 0 else 2 if m32 % 2 == 0 else 1
    if mt == 4 and s == (1, 1) and k[0] * k[1] > 1 and not pad:
        if ((total_pix + 127) // 128) * (m32 // 4) < 8 * 2 * cus:
            mt = 2
    return mt


def tiled_kernel(C, M, k, s, total_pix) -> str:
    """the instantiation conv2d_tiled launches with INFERA_CONV_WS=0 (wide = MT 4, deep = S 2: whole 64-channel blocks)"""
    Cp = (C + 31) // 32 * 32 if padc(C, M) else C
    return f"conv2d_tiled_kernel<{mt_pick(C, M, k, s, total_pix)}, {2 if Cp % 64 == 0 else 1}{', 0, 2' if padc(C, M) else ''}>"


WS_LDS = 160 * 1024 - 256


def ws_kernel(C, M, k):
    """the weight-stationary instantiation INFERA_CONV_WS=2 launches, or None where no slice of the packed weights fits the LDS (or the channels
    are padded): (MT, S, slice bytes)"""
    if padc(C, M):
        return None
    slice32, m32, deep = k[0] * k[1] * C * 32 * 4, M // 32, C % 64 == 0
    if m32 % 4 == 0 and slice32 * 4 <= WS_LDS:
        return f"conv2d_ws_kernel<4, {2 if deep else 1}, 8>"
    if m32 % 2 == 0 and slice32 * 2 <= WS_LDS:
        return f"conv2d_ws_kernel<2, {2 if deep else 1}, 8>"
    if deep and slice32 <= WS_LDS:
        return "conv2d_ws_kernel<1, 2, 8>"
    return None


def ws_grid(M, mt, total_pix, cus: int = CUS):
    """launch_ws: (workgroups of 8 waves per feature slice, 32-pixel tiles) -- a wave takes more than one tile once tiles > 8 x workgroups"""
    slices, ntiles = M // (32 * mt), (total_pix + 31) // 32
    return min(max(1, cus // slices), (ntiles + 7) // 8), ntiles


def split6_supported(C, M, k, groups=1):
    return tiled_supported(C, M, k, groups) and C % 32 == 0 and M % 64 == 0


def split6_tt(M, k) -> bool:
    return k[1] == 3 and M % 128 != 0


def split6_takes_second_input(M) -> bool:
    return M % 128 == 0


def split6_kernel(C, M, k, second: bool = False) -> str:
    if M % 128 == 0:
        return f"conv2d_split6p_kernel[{k[0] * k[1] * (C // 32)} stages{' + second input' if second else ''}]"
    return "conv2d_split6_kernel<2, true>" if split6_tt(M, k) and not second else "conv2d_split6_kernel<2, false>"


def patch_supported(C, M, groups=1) -> bool:
    """conv2d_patch_supported on conv2d_patch_geom (the LDS and patch-extent limits hold for every small case)"""
    return groups == 1 and C <= 8 and (M + 31) // 32 * 32 <= 128 and (M % 32 == 0 or M % 4 == 0)


def patch_kernel(C, M, k, pool: bool = False) -> str:
    """conv2d_patch: MT = M / 32 feature tiles, the k loop compile-time for 19, 10 or 4 groups of eight (c, ky, kx) values, run-time (0) otherwise"""
    k8 = (C * k[0] * k[1] + 7) // 8
    return f"conv2d_patch_kernel<{(M + 31) // 32}, {k8 if k8 in (19, 10, 4) else 0}{', true' if pool else ''}>"


def patch_pool_supported(C, M, conv_ohw, pool_ohw, pool_pad) -> bool:
    """conv2d_patch_pool_supported: MaxPool 3x3 / 2, pads 0 or 1, at most 64 features, no window without a pixel"""
    return (patch_supported(C, M) and M % 32 == 0 and M <= 64 and pool_pad in (0, 1) and (pool_ohw[0] - 1) * 2 - pool_pad < conv_ohw[0] and
            (pool_ohw[1] - 1) * 2 - pool_pad < conv_ohw[1])


def stem_split6_supported(C, M, k, s) -> bool:
    """conv2d_stem_split6_supported: 64 features, a 7-column stride-2 filter, (C kh + 1) / 2 == 11 k-blocks (three channels of seven rows)"""
    return M == 64 and k[1] == 7 and s == (2, 2) and (C * k[0] + 1) // 2 == 11


def depthwise_supported(C, M, groups) -> bool:
    return groups == C and M == C and C % 4 == 0


GENERIC_CAP = 8192  # conv2d_generic_supported: the k table of (C / groups) kh kw 8-byte entries lives in 64 KiB of LDS


def generic_kernel(C, M, groups=1) -> str:
    """conv2d(): feature tiles of 32 per workgroup by Mg = M / groups -- <= 32: 1, <= 64: 2, else 4 with ceil(Mg / 128) workgroups per group"""
    Mg = M // groups
    return f"conv2d_generic_kernel<{1 if Mg <= 32 else 2 if Mg <= 64 else 4}>"


def generic_served(C, M, k, groups=1, nchw_in=False) -> bool:
    """whether a convolution of a channel-quad plan stays on the generic kernel (schedule.cpp assign_conv_kernels): a stem the patch kernel refuses,
    or a layer that is neither tiled nor depthwise"""
    if nchw_in:
        return not patch_supported(C, M, groups)
    return not tiled_supported(C, M, k, groups) and not depthwise_supported(C, M, groups)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

MAP = (5, 7)       # 35 pixels: 1 / 3 / 5 rows = 35 / 105 / 175 pixels -- under one 128-pixel block, one ragged block, two images astride a block edge
ROWS = (1, 3, 5)
MAP2 = (12, 11)    # x 2 rows = 264 pixels
FP32 = {"INFERA_PRECISION": "fp32", "INFERA_CONV_WS": "0"}
ALL = ("grid", "select", "onehot")


def _under_test(name, C, M, k=1, s=1, p=0, d=1, act="", add=False, ohw=MAP, rows=ROWS, env=FP32, kinds=None, expect="conv_tiled_cq", bias=True, g=1):
    """8 -> C 1x1 stem (Relu), then the convolution under test with an `ohw` map; `add`: a residual Add of a second 1x1 branch 8 -> M ... here the
    stem's own output where C == M and the geometry keeps the extent"""
    k, s, d, p = _pair(k), _pair(s), _pair(d), _pads(p)
    hw = in_hw(ohw, k, s, p, d)
    ops = [conv(C, 1, act="Relu"), conv(M, k, s, p, d, g=g, bias=bias, act=act, add=1 if add else None)]
    if kinds is None:
        kinds = ("grid",) if add or act not in ("", "Relu") else ALL
    return {"id": name, "inp": (8, *hw), "ops": ops, "env": dict(env), "expect": ["conv_patch", expect] + (["skipped"] if add else []) + ["convt_phase"],
            "kinds": kinds, "rows": rows}  # (a fused residual Add stays in the plan as a skipped step)


TILED = [
    # feature tiles: M = 32 .. 192 -> MT 1, 2, 3, 4, 1, 3; MT 4 through a 1x1 layer (a small stride-1 3x3 launch falls to MT 2: asserted)
    _under_test("m32-3x3", 32, 32, 3, 1, 1), _under_test("m64-3x3", 32, 64, 3, 1, 1), _under_test("m96-3x3", 32, 96, 3, 1, 1),
    _under_test("m128-1x1", 32, 128, 1), _under_test("m128-3x3-falls-to-mt2", 32, 128, 3, 1, 1), _under_test("m160-1x1", 32, 160, 1),
    _under_test("m192-3x3", 32, 192, 3, 1, 1),
    # channel depth: 32 / 96 (S = 1), 64 / 128 (S = 2), each with MT 1, 2, 3, 4 somewhere
    _under_test("c96-m32-3x3", 96, 32, 3, 1, 1), _under_test("c96-m128-1x1s2", 96, 128, 1, 2), _under_test("c64-m32-3x3", 64, 32, 3, 1, 1),
    _under_test("c64-m64-3x3s2", 64, 64, 3, 2, 1), _under_test("c64-m96-1x1", 64, 96, 1), _under_test("c64-m128-3x3s2", 64, 128, 3, 2, 1),
    _under_test("c128-m64-3x3", 128, 64, 3, 1, 1), _under_test("c128-m128-1x1", 128, 128, 1), _under_test("c96-m96-1x1", 96, 96, 1),
    # padded channels
    _under_test("padc-12-20", 12, 20, 3, 1, 1), _under_test("padc-60-36", 60, 36, 3, 1, 1), _under_test("padc-40-100", 40, 100, 3, 2, 1),
    _under_test("padc-40-100-1x1", 40, 100, 1),
    # filters
    _under_test("1x1s2", 32, 64, 1, 2), _under_test("3x3d2", 32, 64, 3, 1, 2, 2), _under_test("1x3-left", 32, 64, (1, 3), 1, (0, 2, 0, 0)),
    _under_test("3x1-bottom", 32, 64, (3, 1), 1, (0, 0, 2, 0)), _under_test("2x2", 64, 64, 2), _under_test("5x5s2-pads", 32, 64, 5, 2, (2, 1, 0, 2)),
    _under_test("7x7", 32, 32, 7, 1, 3), _under_test("8x8", 32, 32, 8, 1, (3, 4, 4, 3)),
    # the larger map
    _under_test("map2-3x3", 64, 64, 3, 1, 1, ohw=MAP2, rows=(2,)), _under_test("map2-1x1-m128", 32, 128, 1, ohw=MAP2, rows=(2,)),
    _under_test("map2-padc", 12, 20, 3, 2, 1, ohw=MAP2, rows=(2,)),
    # epilogues (grid; Sigmoid and Tanh belong to the bound: GENERIC)
    _under_test("relu", 32, 64, 3, 1, 1, act="Relu", kinds=("grid", "select")), _under_test("leaky", 32, 64, 3, 1, 1, act="LeakyRelu"),
    _under_test("clip", 32, 96, 3, 1, 1, act="Clip"), _under_test("nobias", 32, 64, 3, 1, 1, bias=False),
    _under_test("residual", 64, 64, 3, 1, 1, add=True), _under_test("residual-relu", 64, 64, 3, 1, 1, act="Relu", add=True),
    _under_test("residual-relu-m128", 128, 128, 1, act="Relu", add=True), _under_test("residual-padc", 20, 20, 3, 1, 1, act="Relu", add=True),
]

# every instantiation the table must reach (asserted without a GPU by tests/test_conv_ref.py from the restated rules)
TILED_INSTANCES = {f"conv2d_tiled_kernel<{mt}, {s}>" for mt in (1, 2, 3, 4) for s in (1, 2)} | {
    "conv2d_tiled_kernel<1, 1, 0, 2>", "conv2d_tiled_kernel<2, 2, 0, 2>", "conv2d_tiled_kernel<4, 2, 0, 2>"}

_WS = dict(FP32, INFERA_CONV_WS="2")
WS = [_under_test("ws-" + n, *a, env=_WS, **kw) for n, a, kw in [
    ("4-1", (32, 128, 1), {}), ("4-2", (64, 128, 1, 2), {}), ("2-1", (32, 64, 3, 1, 1), {}), ("2-2", (64, 64, 3, 1, 1), {}),
    ("1-2", (128, 32, 3, 1, 1), {}), ("2-2-residual", (64, 64, 3, 1, 1), {"act": "Relu", "add": True}), ("2-1-map2", (32, 64, 3, 1, 1), {"ohw": MAP2, "rows": (2,)})]]
WS_INSTANCES = {"conv2d_ws_kernel<4, 1, 8>", "conv2d_ws_kernel<4, 2, 8>", "conv2d_ws_kernel<2, 1, 8>", "conv2d_ws_kernel<2, 2, 8>", "conv2d_ws_kernel<1, 2, 8>"}


def ws_wrap_case():
    """the smallest launch with more 32-pixel tiles than the persistent grid has waves: a 32 -> 256 1x1 layer is two 128-feature slices (MT 4), so
    launch_ws gives each CUS / 2 workgroups of 8 waves = CUS * 4 waves; CUS * 4 + 1 tiles wrap.  One image: a (CUS * 4) x 32 + 1 pixel map"""
    tiles = CUS * 4 + 1
    pixels = (tiles - 1) * 32 + 1
    hw = next((h, pixels // h) for h in range(int(pixels ** 0.5), 0, -1) if pixels % h == 0 and h != pixels // h)
    c = _under_test("ws-wrap", 32, 256, 1, ohw=hw, rows=(1,), env=_WS, kinds=("grid", "select"))
    return c, tiles


_DEF = {}  # the default plan: bf16x6
SPLIT = [_under_test("s6-" + n, *a, env=_DEF, expect="conv_split_bf16x6", **kw) for n, a, kw in [
    ("tt-3x3", (32, 64, 3, 1, 1), {}), ("tt-3x3-c64s2", (64, 64, 3, 2, 1), {}), ("tt-1x3", (32, 192, (1, 3), 1, (0, 1, 0, 1)), {}),
    ("plain-1x1", (32, 64, 1), {}), ("plain-5x5", (64, 64, 5, 2, (2, 1, 0, 2)), {}), ("plain-2x2-m192", (32, 192, 2), {}),
    ("p-1stage", (32, 128, 1), {}), ("p-2stages", (64, 128, 1, 2), {}), ("p-3stages", (96, 128, 1), {}), ("p-3x3", (64, 128, 3, 1, 1), {}),
    ("p-3x3-m256-map2", (32, 256, 3, 2, 1), {"ohw": MAP2, "rows": (2,)}), ("tt-residual-relu", (64, 64, 3, 1, 1), {"act": "Relu", "add": True}),
    ("p-leaky", (32, 128, 3, 1, 1), {"act": "LeakyRelu"})]]


def shortcut_case(stride=1):
    """a ResNet block's projection shortcut folded into the block's second convolution as extra K stages (SecondInput): A = stem, P = Relu(conv3x3/s(A)),
    out = Relu(conv3x3(P) + conv1x1/s(A)) -- the 1x1 layer runs last, carries the Add and is folded into the 128-feature launch before it"""
    hw = in_hw(MAP, 3, stride, 1)
    ops = [conv(64, 1, act="Relu"), conv(128, 3, stride, 1, act="Relu"), conv(128, 3, 1, 1), conv(128, 1, stride, src=1, add=3, act="Relu")]
    return {"id": f"s6-folded-shortcut-s{stride}", "inp": (8, *hw), "ops": ops, "env": {}, "kinds": ("grid",), "rows": ROWS,
            "expect": ["conv_patch", "conv_split_bf16x6", "conv_split_bf16x6", "skipped", "skipped", "convt_phase"]}


SPLIT += [shortcut_case(1), shortcut_case(2)]


def _stem(name, C, M, k, s=1, p=0, act="", ohw=MAP, rows=ROWS, env=FP32, tail=None, expect="conv_patch", kinds=ALL, g=1):
    k, s, p = _pair(k), _pair(s), _pads(p)
    ops = [conv(M, k, s, p, g=g, act=act)] + ([tail] if tail else [])
    return {"id": name, "inp": (C, *in_hw(ohw, k, s, p)), "ops": ops, "env": dict(env), "expect": [expect] + (["skipped"] if tail else []) + ["convt_phase"],
            "kinds": kinds, "rows": rows}


STEM = [
    _stem("c1-m32-3x3", 1, 32, 3, 1, 1), _stem("c2-m64-5x5s2", 2, 64, 5, 2, 2), _stem("c3-m32-3x3-k4", 3, 32, 3, 1, 1), _stem("c3-m64-5x5-k10", 3, 64, 5, 1, 2),
    _stem("c3-m96-7x7s2-k19", 3, 96, 7, 2, 3), _stem("c4-m128-3x3s2", 4, 128, 3, 2, 0), _stem("c8-m64-3x3", 8, 64, 3, 1, (1, 0, 0, 1)),
    # (8 channels x 7 x 7 exceed the patch kernel's LDS patch: the planner leaves this stem on the generic kernel, NCHW in, channel quads out -- kept, asserted as such)
    _stem("c8-m128-7x7", 8, 128, 7, 1, (3, 2, 1, 0), expect="normal"), _stem("c4-m20-5x5", 4, 20, 5, 1, 1), _stem("c3-m64-3x3-map2", 3, 64, 3, 2, 1, ohw=MAP2, rows=(2,)),
    _stem("c3-m32-relu", 3, 32, 3, 1, 1, act="Relu", kinds=("grid", "select")),
]


def _stem_pool(name, C, M, k, s, p, pooled, ppad, ceil, env=FP32, expect="conv_patch_pool", rows=(1, 3), kinds=ALL):
    """stem -> MaxPool 3x3 / 2 with `pooled` outputs: the convolution's extent is the smallest (ceil_mode: the largest) that pools to it"""
    k, s, p = _pair(k), _pair(s), _pads(p)
    conv_hw = tuple((pooled[a] - 1) * 2 + 3 - 2 * ppad - (1 if ceil else 0) for a in range(2))
    assert out_hw(conv_hw, 3, 2, ppad, 1, ceil) == tuple(pooled), (conv_hw, pooled)
    return _stem(name, C, M, k, s, p, ohw=conv_hw, rows=rows, env=env, tail=pool("max", 3, 2, ppad, ceil=ceil), expect=expect, kinds=kinds)


# the pooled tile is 8 x 7: extents one below, equal to and one above it; no Relu, so negative values reach the pool
STEM_POOL = [
    _stem_pool("pool-7x6-pad0", 3, 32, 3, 1, 1, (7, 6), 0, False), _stem_pool("pool-8x7-pad1", 3, 64, 3, 1, 1, (8, 7), 1, False),
    _stem_pool("pool-9x8-pad1-ceil", 3, 32, 5, 1, 2, (9, 8), 1, True), _stem_pool("pool-8x7-pad0-ceil", 4, 64, 3, 2, 1, (8, 7), 0, True),
    _stem_pool("pool-9x8-c8-runtime-k", 8, 64, 3, 1, 1, (9, 8), 0, False),
    _stem_pool("pool2-7x7s2", 3, 64, 7, 2, 3, (9, 8), 1, False, env=dict(FP32, INFERA_STEM_POOL2="2")),
    _stem_pool("pool2-5x5", 3, 64, 5, 1, 2, (8, 7), 1, False, env=dict(FP32, INFERA_STEM_POOL2="2")),
    _stem_pool("pool2-off-7x7s2", 3, 64, 7, 2, 3, (9, 8), 1, False, env=dict(FP32, INFERA_STEM_POOL2="0")),
    _stem_pool("stem-split6-7x7s2", 3, 64, 7, 2, 3, (9, 8), 1, False, env={}, expect="conv_patch_pool_bf16x6"),
    _stem_pool("stem-split6-7x7s2-ceil", 3, 64, 7, 2, 3, (8, 9), 0, True, env={}, expect="conv_patch_pool_bf16x6"),
]


def _neighbour(name, C, ohw, tail, expect, rows=(1, 3), env=FP32, kinds=("grid", "select"), expect_tail=None):
    """3 -> C 1x1 stem, then the channel-quad operator(s) `tail` on an `ohw` map"""
    return {"id": name, "inp": (3, *ohw), "ops": [conv(C, 1)] + list(tail), "env": dict(env), "expect": ["conv_patch"] + list(expect), "kinds": kinds, "rows": rows}


def _dw(C, k, s, p):
    return conv(C, k, s, p, g=C)


NEIGHBOURS = [
    # depthwise: planes <= 64 pixels (64-thread blocks) and > 256 pixels (256-thread blocks, two of them)
    _neighbour("dw-3x3-small", 8, (7, 9), [_dw(8, 3, 1, 1)], ["conv_depthwise", "convt_phase"]),
    _neighbour("dw-5x5s2-small", 12, (11, 13), [_dw(12, 5, 2, 2)], ["conv_depthwise", "convt_phase"]),
    _neighbour("dw-3x3s2-large", 8, (37, 31), [_dw(8, 3, 2, 1)], ["conv_depthwise", "convt_phase"]),
    _neighbour("dw-5x5-large", 4, (17, 19), [_dw(4, 5, 1, 2)], ["conv_depthwise", "convt_phase"]),
    # max pools with compile-time windows, and the generic channel-quad pool
    _neighbour("max3x3s2", 8, (11, 13), [pool("max", 3, 2, 1)], ["normal", "convt_phase"]),
    _neighbour("max2x2s2-ceil", 8, (11, 13), [pool("max", 2, 2, 0, ceil=True)], ["normal", "convt_phase"]),
    _neighbour("max3x3s1-large", 4, (19, 17), [pool("max", 3, 1, 1)], ["normal", "convt_phase"]),
    _neighbour("max3x3d2", 8, (11, 13), [pool("max", 3, 1, 2, d=2)], ["normal", "convt_phase"]),
    _neighbour("max2x3-large", 4, (19, 17), [pool("max", (2, 3), 1, (1, 0, 0, 2))], ["normal", "convt_phase"]),
    _neighbour("gmp", 12, (5, 7), [{"op": "gmp"}], ["normal"]),
    _neighbour("gap", 12, (8, 8), [{"op": "gap"}], ["normal"], kinds=("grid",)),  # (64 pixels: the mean of integers is exact)
    # data movement
    _neighbour("concat", 8, (5, 7), [conv(12, 1, src=0), {"op": "concat", "srcs": [1, 2, 1]}], ["conv_patch", "normal", "normal", "normal", "convt_phase"]),  # (one copy per piece)
    _neighbour("slice", 16, (5, 7), [{"op": "slice", "c0": 4, "c1": 12}], ["normal", "convt_phase"]),
    _neighbour("shuffle", 24, (5, 7), [{"op": "shuffle", "groups": 3}], ["normal", "convt_phase"]),
]

# average pools on a grid: the window's sum of small integers is exact in any order and the division (pool2d_cq_kernel divides, it does not multiply
# by a reciprocal) one correctly rounded f32 operation -- compared bit for bit with the f32 quotient of the exact sum (avg_exact).  ceil_mode with
# count_include_pad is refused at load time (lowering.cpp), so the two are covered apart.
AVG = [
    _neighbour("avg3x3s2", 8, (11, 13), [pool("avg", 3, 2, 1)], ["normal", "convt_phase"], kinds=("grid",)),
    _neighbour("avg3x3s2-cip", 8, (11, 13), [pool("avg", 3, 2, (1, 0, 1, 2), cip=True)], ["normal", "convt_phase"], kinds=("grid",)),
    _neighbour("avg3x3s2-ceil", 8, (12, 14), [pool("avg", 3, 2, 1, ceil=True)], ["normal", "convt_phase"], kinds=("grid",)),
    _neighbour("avg2x2-large", 4, (19, 17), [pool("avg", 2, 1, (0, 1, 1, 0))], ["normal", "convt_phase"], kinds=("grid",)),
]


def avg_exact(case, weights, x):
    """the one right f32 answer of a grid case that ends in an average pool: f32(exact sum) / f32(divisor)"""
    o = case["ops"][-1]
    assert o["op"] == "avgpool"
    h = forward64(dict(case, ops=case["ops"][:-1]), weights, x)["out"]
    sums, cnt = pool64(h, "avg", o["k"], o["s"], o["p"], o["d"], o["ceil"], o["cip"], parts=True)
    assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums) and np.abs(sums).max() < 2 ** 24
    return sums.astype(np.float32) / cnt.astype(np.float32)[None, None]

# generic data: one case per family (synth.table values and the cancelling 1000 +- 1 variant), Sigmoid and Tanh among the epilogues
GENERIC = [
    _under_test("g-tiled-3x3", 64, 64, 3, 1, 1, act="Relu", rows=(3,)), _under_test("g-tiled-1x1-sigmoid", 32, 128, 1, act="Sigmoid", rows=(3,)),
    _under_test("g-tiled-padc-tanh", 40, 100, 3, 2, 1, act="Tanh", rows=(3,)), _under_test("g-tiled-residual", 64, 64, 3, 1, 1, act="Relu", add=True, rows=(3,)),
    _under_test("g-ws", 64, 64, 3, 1, 1, env=_WS, rows=(3,)),
    _under_test("g-s6-tt", 64, 64, 3, 1, 1, env=_DEF, expect="conv_split_bf16x6", rows=(3,)),
    _under_test("g-s6-plain", 64, 64, 5, 2, (2, 1, 0, 2), env=_DEF, expect="conv_split_bf16x6", rows=(3,)),
    _under_test("g-s6-p", 96, 128, 3, 1, 1, act="Relu", env=_DEF, expect="conv_split_bf16x6", rows=(3,)),
    _stem("g-stem-7x7s2", 3, 96, 7, 2, 3, rows=(3,)), _stem_pool("g-stem-pool", 3, 64, 5, 1, 2, (8, 7), 1, False, rows=(3,)),
    _stem_pool("g-stem-split6", 3, 64, 7, 2, 3, (9, 8), 1, False, env={}, expect="conv_patch_pool_bf16x6", rows=(3,)),
    _neighbour("g-depthwise", 8, (11, 13), [_dw(8, 3, 1, 1)], ["conv_depthwise", "convt_phase"], rows=(3,)),
]


# ---- conv2d_generic_kernel<MT> and the NCHW forms of its neighbours (tests/test_conv_generic_gpu.py) -----------------------------------

def _plain(case, expect=None):
    """the case served as the tensor itself: an NCHW plan, every step on the generic kernels"""
    return dict(case, probe="", layout="NCHW", expect=expect)  # (expect None: every exec kind "normal", however many steps)


def _nchw(name, C, M, k=3, s=1, p=1, d=1, g=1, act="", bias=True, ohw=MAP, rows=ROWS, kinds=None):
    """ONE convolution of the caller's NCHW input, served as it is"""
    k, s, d, p = _pair(k), _pair(s), _pair(d), _pads(p)
    if kinds is None:
        kinds = ALL if act in ("", "Relu") and bias else ("grid",)
    return _plain({"id": name, "inp": (C, *in_hw(ohw, k, s, p, d)), "ops": [conv(M, k, s, p, d, g=g, bias=bias, act=act)], "env": dict(FP32), "kinds": kinds, "rows": rows})


GENERIC_NCHW = [
    # feature tiles by Mg: <1> to 32, <2> to 64, <4> beyond with ceil(Mg / 128) workgroups per group; 33, 65 and 132 leave a tile almost empty
    *[_nchw(f"nchw-m{M}", 6, M, rows=(1, 3) if M > 128 else ROWS) for M in (1, 5, 32, 33, 64, 65, 128, 132, 160)],
    # the k loop takes two taps per step: an odd KK = Cg kh kw and KK = 1 leave the upper lane half on the k < KK guard alone
    _nchw("nchw-kk27", 3, 8), _nchw("nchw-kk1", 1, 8, 1, p=0), _nchw("nchw-kk5", 5, 8, 1, p=0),
    # the receptive field: the corner pointer before the image, guarded by the (iy, ix) test alone
    _nchw("nchw-3x3d2", 6, 8, 3, 1, 2, 2), _nchw("nchw-5x5s2-pads", 6, 8, 5, 2, (2, 1, 0, 2)), _nchw("nchw-1x3-left", 6, 8, (1, 3), 1, (0, 2, 0, 0)),
    _nchw("nchw-3x1-bottom", 6, 8, (3, 1), 1, (0, 0, 2, 0)), _nchw("nchw-9x9-larger-than-the-map", 6, 8, 9, 1, 4), _nchw("nchw-2x2", 6, 8, 2, 1, 0),
    # groups: Cg = Mg = 2; Cg = 4, Mg = 6; a depth multiplier of 2; depthwise where the plan is NCHW
    _nchw("nchw-g3-c6-m6", 6, 6, g=3), _nchw("nchw-g3-c12-m18", 12, 18, g=3), _nchw("nchw-g5-c5-m10", 5, 10, g=5), _nchw("nchw-g6-depthwise", 6, 6, g=6),
    # epilogues (grid; Sigmoid and Tanh belong to the bound: GENERIC_G)
    _nchw("nchw-relu", 6, 8, act="Relu", kinds=("grid",)), _nchw("nchw-leaky", 6, 8, act="LeakyRelu"), _nchw("nchw-clip", 6, 8, act="Clip"),
    _nchw("nchw-nobias", 6, 8, bias=False, kinds=("grid",)),
    # the LDS cap: KK = 512 x 4 x 4 = 8192 entries of 8 bytes are the whole 64 KiB (no lattice of lit pixels on a 4 x 4 image under a 4 x 4 filter: no onehot)
    # (a [4, 1, 1] result has no layout to keep NCHW: the plan is in channel quads, its one step the generic kernel with NCHW in and one quad out)
    dict(_nchw("nchw-kk8192-cap", 512, 4, 4, 1, 0, ohw=(1, 1), rows=(1, 3), kinds=("grid", "select")), layout="NC/4HW4", expect=["normal"]),
]
OVER_CAP = dict(_nchw("nchw-kk8256-over-the-cap", 516, 4, 4, 1, 0, ohw=(1, 1), rows=(1,), kinds=("grid",)), layout="NC/4HW4", expect=["normal"])


def _quads(name, C, M, k=3, p=1, g=1, kinds=ALL, rows=ROWS):
    """8 -> C 1x1 stem, then the convolution under test, which the fast channel-quad kernels refuse"""
    return dict(_under_test(name, C, M, k, 1, p, g=g, kinds=kinds, rows=rows, expect="normal"), probe="A", layout="NC/4HW4")


GENERIC_CQ_GROUPED = [
    _quads("cq-g4-c8-m8-shared-quads", 8, 8, g=4),             # Cg = Mg = 2: two groups in one input quad, scalar stores into quads two groups share
    _quads("cq-g4-c24-m24-straddling", 24, 24, g=4),           # Cg = Mg = 6: groups straddle quads on both sides
    _quads("cq-g4-c16-m16-quad-store", 16, 16, g=4),           # Mg = 4: the 16-byte store at grp * Mg + ml
    _quads("cq-g2-c32-m256-mt4", 32, 256, g=2, rows=(1, 3)),   # Mg = 128: <4>, one full workgroup of features per group
    _quads("cq-g2-c8-m264-two-tiles", 8, 264, g=2, rows=(1, 3)),  # Mg = 132: two feature workgroups per group, the second almost empty
    _quads("cq-g8-c8-m16-depth-multiplier", 8, 16, g=8),       # groups == C, M == 2 C: not the depthwise kernel's
]
GENERIC_CQ = GENERIC_CQ_GROUPED + [
    _quads("cq-9x9-81-taps", 8, 8, 9, 4),                      # more than the tiled kernel's 64-bit tap mask
    # stems the patch kernel refuses: NCHW in, channel quads out
    dict(_stem("cq-stem-c12-m32", 12, 32, 3, 1, 1, expect="normal"), probe="A", layout="NC/4HW4"),
    dict(_stem("cq-stem-c3-m160", 3, 160, 3, 1, 1, expect="normal", rows=(1, 3)), probe="A", layout="NC/4HW4"),
    dict(_stem("cq-stem-c4-m32-g2", 4, 32, 3, 1, 1, expect="normal", g=2), probe="A", layout="NC/4HW4"),
    # the head: a 1x1 convolution with 10 features on the [C, 1, 1] of a global pool (8 x 8: an exact mean), stored in plain order
    {"id": "cq-head-m10", "inp": (3, 8, 8), "ops": [conv(12, 1), {"op": "gap"}, conv(10, 1)], "env": dict(FP32), "expect": ["conv_patch", "normal", "normal"],
     "kinds": ("grid",), "rows": (1, 3), "probe": "A", "layout": "NC/4HW4"},
]


def _neighbour_nchw(name, C, ohw, tail, kinds=("grid", "select"), rows=(1, 3)):
    """3 -> C 1x1 stem with C no multiple of 4 (or a slice off a quad boundary), so that the plan is NCHW, then `tail`; served as it is"""
    return _plain(_neighbour(name, C, ohw, tail, [], rows=rows, kinds=kinds))


# the geometries of NEIGHBOURS and AVG on pool2d_kernel, the NCHW branches of global_avgpool_kernel, copy_cols and channel_shuffle_planes_kernel<false>
NEIGHBOURS_NCHW = [
    _neighbour_nchw("nchw-max3x3s2", 6, (11, 13), [pool("max", 3, 2, 1)]), _neighbour_nchw("nchw-max2x2s2-ceil", 6, (11, 13), [pool("max", 2, 2, 0, ceil=True)]),
    _neighbour_nchw("nchw-max3x3d2", 6, (11, 13), [pool("max", 3, 1, 2, d=2)]), _neighbour_nchw("nchw-max2x3-pads", 6, (19, 17), [pool("max", (2, 3), 1, (1, 0, 0, 2))]),
    _neighbour_nchw("nchw-gmp", 6, (5, 7), [{"op": "gmp"}]), _neighbour_nchw("nchw-gap", 6, (8, 8), [{"op": "gap"}], kinds=("grid",)),
    _neighbour_nchw("nchw-concat", 6, (5, 7), [conv(12, 1, src=0), {"op": "concat", "srcs": [1, 2, 1]}]),
    _neighbour_nchw("nchw-slice-off-quad", 8, (5, 7), [{"op": "slice", "c0": 2, "c1": 6}]),  # channels 2..5 of 8
    _neighbour_nchw("nchw-shuffle", 6, (5, 7), [{"op": "shuffle", "groups": 3}]),
]
AVG_NCHW = [
    _neighbour_nchw("nchw-avg3x3s2", 6, (11, 13), [pool("avg", 3, 2, 1)], kinds=("grid",)),
    _neighbour_nchw("nchw-avg3x3s2-cip", 6, (11, 13), [pool("avg", 3, 2, (1, 0, 1, 2), cip=True)], kinds=("grid",)),
    _neighbour_nchw("nchw-avg3x3s2-ceil", 6, (12, 14), [pool("avg", 3, 2, 1, ceil=True)], kinds=("grid",)),
]


def _per_channel(name, C, tail, expect, ohw=MAP, kinds=(), rows=(1, 3)):
    """3 -> C 1x1 stem, then the per-channel operator(s): served in channel quads through probe A and, as_nchw(), in NCHW as it is"""
    return dict(_neighbour(name, C, ohw, tail, expect, rows=rows, kinds=kinds), probe="A", layout="NC/4HW4")


def as_nchw(case):
    return _plain(case)


def lrn_identity(case):
    """the LRN case with alpha = 0 and bias = 1: pow(1, beta) == 1, y == x to the bit -- pins the element index in either layout"""
    return dict(case, id=case["id"] + "-identity", ops=[dict(o, alpha=0.0, bias=1.0) if o["op"] == "lrn" else o for o in case["ops"]], kinds=("grid", "select"))


_PC = ["normal", "convt_phase"]
# LRN with an alpha that matters (AlexNet's 1e-4 would hide a wrong window under the bar); generic data and the layout identity only (kinds ())
LRN = [
    _per_channel("lrn-size3", 8, [lrn(3, 1.0, 0.75, 1.0)], _PC), _per_channel("lrn-size5", 8, [lrn(5, 2.0, 0.5, 2.0)], _PC),
    _per_channel("lrn-size5-c4-clipped-both-ends", 4, [lrn(5, 1.0, 0.75, 1.0)], _PC), _per_channel("lrn-size4-even", 8, [lrn(4, 1.5, 0.75, 1.0)], _PC),
]
PER_CHANNEL_EXACT = [lrn_identity(c) for c in LRN] + [
    # squeeze and excitation on an 8 x 8 map (an exact mean): stem, gap, 1x1 convolution, stem * gate
    _per_channel("gate", 8, [{"op": "gap"}, conv(8, 1, src=2), gate(1, 3)], ["normal", "conv_tiled_cq", "normal", "convt_phase"], ohw=(8, 8), kinds=("grid",)),
    # a BatchNormalization behind a max pool cannot fold into a convolution: an AffineChannel step
    _per_channel("bn-behind-maxpool", 8, [pool("max", 3, 2, 1), bn()], ["normal", "normal", "convt_phase"], ohw=(11, 13), kinds=("grid",)),
]
PER_CHANNEL = LRN + [
    _per_channel("g-gate-sigmoid", 8, [{"op": "gap"}, conv(8, 1, src=2, act="Sigmoid"), gate(1, 3)], ["normal", "conv_tiled_cq", "normal", "convt_phase"], ohw=(8, 8)),
    _per_channel("g-bn-behind-maxpool", 8, [pool("max", 3, 2, 1), bn()], ["normal", "normal", "convt_phase"], ohw=(11, 13)),
]

# generic data on the generic kernel: NCHW groups 1, grouped in quads, 9x9, a depth multiplier, the Sigmoid and Tanh epilogues
GENERIC_G = [
    dict(_nchw("g-nchw-m65", 6, 65, act="Relu", rows=(3,)), kinds=()), dict(_nchw("g-nchw-sigmoid", 6, 33, act="Sigmoid", rows=(3,)), kinds=()),
    dict(_nchw("g-nchw-g3-tanh", 12, 18, g=3, act="Tanh", rows=(3,)), kinds=()),
    dict(_quads("g-cq-g4-c24-m24", 24, 24, g=4, rows=(3,)), kinds=()), dict(_quads("g-cq-9x9", 8, 8, 9, 4, rows=(3,)), kinds=()),
    dict(_quads("g-cq-depth-multiplier", 8, 16, g=8, rows=(3,)), kinds=()),
]


def generic_weights(case, seed: int = 31):
    """U(-1, 1) / sqrt(fan-in) weights and U(-0.1, 0.1) biases"""
    rng = np.random.default_rng([seed, *case["inp"]])
    sh, out = shapes(case), {}
    for i, o in enumerate(case["ops"]):
        if o["op"] == "bn":
            out[i] = (rng.uniform(0.5, 2.0, sh[i + 1][0]).astype(np.float32) * rng.choice([-1, 1], sh[i + 1][0]).astype(np.float32), rng.uniform(-1, 1, sh[i + 1][0]).astype(np.float32))
        if o["op"] != "conv":
            continue
        Cg = sh[o["src"] if o.get("src") is not None else i][0] // o["g"]
        fan = Cg * o["k"][0] * o["k"][1]
        out[i] = ((rng.uniform(-1, 1, (o["M"], Cg, *o["k"])) / np.sqrt(fan)).astype(np.float32), rng.uniform(-0.1, 0.1, o["M"]).astype(np.float32) if o["bias"] else None)
    return out


def generic_inputs(case, rows: int):
    """synth.table's uniform [-1, 1) values, and 1000 +- 1: sums that cancel"""
    from infera_amd import synth

    n = int(np.prod(case["inp"]))
    return {"uniform": synth.table(21, 0, rows, n), "offset": (1000 + np.random.default_rng(n).uniform(-1, 1, (rows, n))).astype(np.float32)}


def conv_under_test(case):
    """(C, M, k, s) of the case's second convolution (the one behind the stem)"""
    o = case["ops"][1]
    return case["ops"][0]["M"], o["M"], o["k"], o["s"]


def total_pix(case, rows):
    sh = shapes(case)
    return rows * sh[2][1] * sh[2][2]


def set_env(env):
    """the knobs of a case around load_model / predict: returns what to hand to restore_env"""
    import os

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    return old


def restore_env(old):
    import os

    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
