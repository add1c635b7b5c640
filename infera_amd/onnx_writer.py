"""Minimal ONNX protobuf writer (no `onnx` package in this image).

Emits ModelProto files for the benchmark / parity configurations of BASELINE.md section 4:
a dynamic-batch twin of the reference's ``linear.onnx`` fixture, the C2/C3 MLP
(Gemm+Relu chain), the C4 logistic-regression + Softmax model and the C5 ResNet-18 topology.
All models carry a symbolic batch dimension ``N`` so a whole DuckDB vector (<=2048 rows) or
a super-batch goes through in one call (the reference's fixture has a fixed batch of 1,
/root/reference test/models/README.md:5).

Wire format follows onnx.proto3 field numbers (ModelProto.graph=7, GraphProto.node=1 ...).
Weights are written as ``raw_data`` (little-endian f32) unless ``float_data=True`` which
reproduces the encoding of the reference fixture (packed field 4).
"""
from __future__ import annotations

import math
import struct
from typing import Iterable, Sequence

import numpy as np

from .synth import uniform_pm1

FLOAT = 1
INT64 = 7


def _varint(v: int) -> bytes:
    if v < 0:
        v += 1 << 64
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _tag(field: int, wt: int) -> bytes:
    return _varint((field << 3) | wt)


def _ld(field: int, payload: bytes) -> bytes:
    return _tag(field, 2) + _varint(len(payload)) + payload


def _vi(field: int, v: int) -> bytes:
    return _tag(field, 0) + _varint(v)


def _s(field: int, s: str) -> bytes:
    return _ld(field, s.encode())


UINT8, INT8, INT32 = 2, 3, 6
BOOL = 9
FLOAT16, BFLOAT16 = 10, 16
_SMALL_INTS = {np.dtype(np.uint8): (UINT8, "u1"), np.dtype(np.int8): (INT8, "i1"), np.dtype(np.int32): (INT32, "<i4")}


def tensor(name: str, arr: np.ndarray, float_data: bool = False, int32_data: bool = False) -> bytes:
    """TensorProto: dims=1, data_type=2, float_data=4, int32_data=5, int64_data=7, name=8, raw_data=9.  uint8 / int8 / int32 arrays
    (quantised graphs) go into raw_data, or one varint each into int32_data."""
    arr = np.asarray(arr)
    out = b"".join(_vi(1, int(d)) for d in arr.shape)
    if arr.dtype in _SMALL_INTS:
        code, fmt = _SMALL_INTS[arr.dtype]
        out += _vi(2, code)
        if int32_data:
            out += _ld(5, b"".join(_varint(int(v)) for v in arr.reshape(-1)))
        else:
            out += _ld(9, arr.astype(fmt).tobytes())
        return out + _s(8, name)
    if arr.dtype == np.bool_:  # one byte per element in raw_data, or one int32 each in int32_data
        out += _vi(2, BOOL)
        if int32_data:
            out += _ld(5, b"".join(_varint(int(v)) for v in arr.reshape(-1)))
        else:
            out += _ld(9, arr.astype("u1").tobytes())
        return out + _s(8, name)
    if arr.dtype == np.float16:  # two bytes per element in raw_data, or one 16-bit pattern per element in int32_data
        out += _vi(2, FLOAT16)
        if int32_data:
            out += _ld(5, b"".join(_varint(int(v)) for v in arr.reshape(-1).view(np.uint16)))
        else:
            out += _ld(9, arr.astype("<f2").tobytes())
        return out + _s(8, name)
    if arr.dtype == np.float32:
        out += _vi(2, FLOAT)
        if float_data:
            out += _ld(4, arr.astype("<f4").tobytes())
        else:
            out += _ld(9, arr.astype("<f4").tobytes())
    elif arr.dtype == np.int64:
        out += _vi(2, INT64)
        out += _ld(9, arr.astype("<i8").tobytes())
    else:
        raise TypeError(arr.dtype)
    return out + _s(8, name)


def attr_i(name: str, v: int) -> bytes:
    return _s(1, name) + _vi(3, v) + _vi(20, 2)


def attr_f(name: str, v: float) -> bytes:
    return _s(1, name) + _tag(2, 5) + struct.pack("<f", v) + _vi(20, 1)


def attr_ints(name: str, vs: Iterable[int]) -> bytes:
    return _s(1, name) + b"".join(_vi(8, int(v)) for v in vs) + _vi(20, 7)


def attr_s(name: str, v: str) -> bytes:
    return _s(1, name) + _ld(4, v.encode()) + _vi(20, 3)


def attr_floats(name: str, vs: Iterable[float]) -> bytes:
    return _s(1, name) + b"".join(_tag(7, 5) + struct.pack("<f", float(v)) for v in vs) + _vi(20, 6)


def attr_strings(name: str, vs: Iterable[str]) -> bytes:
    return _s(1, name) + b"".join(_ld(9, v.encode()) for v in vs) + _vi(20, 8)


ML_DOMAIN = "ai.onnx.ml"


def node(op: str, inputs: Sequence[str], outputs: Sequence[str], attrs: Sequence[bytes] = (), name: str = "",
         domain: str = "") -> bytes:
    out = b"".join(_s(1, i) for i in inputs) + b"".join(_s(2, o) for o in outputs)
    if name:
        out += _s(3, name)
    out += _s(4, op)
    out += b"".join(_ld(5, a) for a in attrs)
    if domain:
        out += _s(7, domain)
    return out


def value_info(name: str, dims: Sequence[int | str], elem_type: int = FLOAT) -> bytes:
    shape = b""
    for d in dims:
        dim = _s(2, d) if isinstance(d, str) else _vi(1, int(d))
        shape += _ld(1, dim)
    ttype = _vi(1, elem_type) + _ld(2, shape)
    return _s(1, name) + _ld(2, _ld(1, ttype))


def model(graph_name: str, nodes: Sequence[bytes], inits: Sequence[bytes], inputs: Sequence[bytes],
          outputs: Sequence[bytes], opset: int = 13, ir_version: int = 8, producer: str = "infera_amd",
          ml_opset: int | None = None) -> bytes:
    g = b"".join(_ld(1, n) for n in nodes) + _s(2, graph_name)
    g += b"".join(_ld(5, t) for t in inits)
    g += b"".join(_ld(11, i) for i in inputs) + b"".join(_ld(12, o) for o in outputs)
    opset_import = _ld(8, _s(1, "") + _vi(2, opset))
    if ml_opset is not None:  # the classical-ML operator domain sklearn exporters use
        opset_import += _ld(8, _s(1, ML_DOMAIN) + _vi(2, ml_opset))
    return _vi(1, ir_version) + _s(2, producer) + _ld(7, g) + opset_import


# ------------------------------------------------------------------------------------------
# deterministic weights: U(-1/sqrt(fan_in), 1/sqrt(fan_in)), seed 1234
# ------------------------------------------------------------------------------------------

class _WeightStream:
    def __init__(self, seed: int = 1234):
        self.seed = seed
        self.counter = 0

    def take(self, shape: Sequence[int], fan_in: int) -> np.ndarray:
        n = int(np.prod(shape))
        idx = np.arange(self.counter, self.counter + n, dtype=np.uint64)
        self.counter += n
        u = uniform_pm1(self.seed, idx).astype(np.float64)
        return (u / math.sqrt(fan_in)).astype(np.float32).reshape(shape)


def linear_dyn() -> bytes:
    """Dynamic-batch twin of the reference fixture test/models/linear.onnx: Y = X.W + B with
    W=(2,-1,0.5), B=0.25 -> (1,2,3) -> 1.75 (test/sql/test_core_functionality.test:48-56)."""
    w = np.array([[2.0], [-1.0], [0.5]], np.float32)
    b = np.array([0.25], np.float32)
    nodes = [node("MatMul", ["X", "W"], ["Z"]), node("Add", ["Z", "B"], ["Y"])]
    return model("LinearModelDyn", nodes, [tensor("W", w, float_data=True), tensor("B", b, float_data=True)],
                 [value_info("X", ["N", 3])], [value_info("Y", ["N", 1])])


def mlp(dims: Sequence[int] = (128, 256, 64, 1), acts: Sequence[str] | None = None, final_softmax: bool = False,
        seed: int = 1234, use_matmul_add: bool = False, trans_b: bool = False, opset: int = 13,
        batch: int | str = "N") -> bytes:
    """Gemm chain `dims[0] -> dims[1] -> ...` with an activation after every layer but the last
    (default Relu; names from {"Relu","Sigmoid","Tanh","LeakyRelu",""}).  C2/C3 = defaults."""
    nl = len(dims) - 1
    if acts is None:
        acts = ["Relu"] * (nl - 1) + [""]
    assert len(acts) == nl
    ws = _WeightStream(seed)
    nodes, inits = [], []
    cur = "X"
    for l in range(nl):
        k, m = dims[l], dims[l + 1]
        w = ws.take((k, m), k)
        b = ws.take((m,), k)
        out = f"H{l}" if (l < nl - 1 or acts[l] or final_softmax) else "Y"
        if use_matmul_add:
            inits += [tensor(f"W{l}", w), tensor(f"B{l}", b)]
            nodes += [node("MatMul", [cur, f"W{l}"], [f"Z{l}"]), node("Add", [f"Z{l}", f"B{l}"], [out])]
        elif trans_b:
            inits += [tensor(f"W{l}", np.ascontiguousarray(w.T)), tensor(f"B{l}", b)]
            nodes += [node("Gemm", [cur, f"W{l}", f"B{l}"], [out], [attr_i("transB", 1)])]
        else:
            inits += [tensor(f"W{l}", w), tensor(f"B{l}", b)]
            nodes += [node("Gemm", [cur, f"W{l}", f"B{l}"], [out])]
        cur = out
        if acts[l]:
            last = l == nl - 1 and not final_softmax
            out = "Y" if last else f"A{l}"
            attrs = [attr_f("alpha", 0.1)] if acts[l] == "LeakyRelu" else []
            nodes.append(node(acts[l], [cur], [out], attrs))
            cur = out
    if final_softmax:
        nodes.append(node("Softmax", [cur], ["Y"], [attr_i("axis", 1)]))
    return model("mlp_" + "x".join(map(str, dims)), nodes, inits, [value_info("X", [batch, dims[0]])],
                 [value_info("Y", [batch, dims[-1]])], opset=opset)


def logreg_softmax(features: int = 128, classes: int = 10, seed: int = 1234) -> bytes:
    """C4: Gemm(features -> classes) + Softmax(axis=1)."""
    return mlp((features, classes), acts=[""], final_softmax=True, seed=seed)


def identity(cols: int = 4, batch: int | str = "N") -> bytes:
    return model("identity_dyn", [node("Identity", ["X"], ["Y"])], [], [value_info("X", [batch, cols])],
                 [value_info("Y", [batch, cols])], opset=13)


def resnet18(classes: int = 1000, seed: int = 1234, in_hw: int = 224, width: int = 64) -> bytes:
    """C5: ResNet-18 topology (conv7x7/2 + BN + Relu + maxpool3x3/2, 4 stages x 2 BasicBlocks,
    global-avgpool, Flatten, Gemm -> classes), random weights, BatchNormalization kept as
    separate nodes so the loader's BN-fold is exercised.  Input [N,3,in_hw,in_hw]."""
    ws = _WeightStream(seed)
    nodes, inits = [], []
    uid = [0]

    def fresh(p: str) -> str:
        uid[0] += 1
        return f"{p}{uid[0]}"

    def conv_bn(x: str, cin: int, cout: int, k: int, stride: int, pad: int, relu: bool) -> str:
        w = ws.take((cout, cin, k, k), cin * k * k)
        wn, y = fresh("w"), fresh("c")
        inits.append(tensor(wn, w))
        nodes.append(node("Conv", [x, wn], [y], [attr_ints("kernel_shape", [k, k]), attr_ints("strides", [stride, stride]),
                                                 attr_ints("pads", [pad] * 4)]))
        scale = (1.0 + 0.1 * ws.take((cout,), 1)).astype(np.float32)
        beta = (0.1 * ws.take((cout,), 1)).astype(np.float32)
        mean = (0.1 * ws.take((cout,), 1)).astype(np.float32)
        var = (1.0 + 0.5 * np.abs(ws.take((cout,), 1))).astype(np.float32)
        names = [fresh("bn_s"), fresh("bn_b"), fresh("bn_m"), fresh("bn_v")]
        for nme, arr in zip(names, (scale, beta, mean, var)):
            inits.append(tensor(nme, arr))
        z = fresh("b")
        nodes.append(node("BatchNormalization", [y] + names, [z], [attr_f("epsilon", 1e-5)]))
        if relu:
            r = fresh("r")
            nodes.append(node("Relu", [z], [r]))
            return r
        return z

    x = conv_bn("X", 3, width, 7, 2, 3, True)
    p = fresh("p")
    nodes.append(node("MaxPool", [x], [p], [attr_ints("kernel_shape", [3, 3]), attr_ints("strides", [2, 2]), attr_ints("pads", [1, 1, 1, 1])]))
    x, cin = p, width
    for stage, cout in enumerate([width, width * 2, width * 4, width * 8]):
        for blk in range(2):
            stride = 2 if (stage > 0 and blk == 0) else 1
            y = conv_bn(x, cin, cout, 3, stride, 1, True)
            y = conv_bn(y, cout, cout, 3, 1, 1, False)
            sc = x
            if stride != 1 or cin != cout:
                sc = conv_bn(x, cin, cout, 1, stride, 0, False)
            s, r = fresh("s"), fresh("r")
            nodes.append(node("Add", [y, sc], [s]))
            nodes.append(node("Relu", [s], [r]))
            x, cin = r, cout
    g, f = fresh("g"), fresh("f")
    nodes.append(node("GlobalAveragePool", [x], [g]))
    nodes.append(node("Flatten", [g], [f], [attr_i("axis", 1)]))
    w = ws.take((cin, classes), cin)
    b = ws.take((classes,), cin)
    inits += [tensor("fc_w", w), tensor("fc_b", b)]
    nodes.append(node("Gemm", [f, "fc_w", "fc_b"], ["Y"]))
    return model("resnet18", nodes, inits, [value_info("X", ["N", 3, in_hw, in_hw])], [value_info("Y", ["N", classes])], opset=13)


def unary_zoo(features: int = 16) -> bytes:
    """Every elementwise operator of the breadth set in one graph: a Gemm feeds parallel branches (one per
    operator, inputs pre-conditioned where the domain needs it), the branches are concatenated (axis 1)."""
    ws = _WeightStream(77)
    w = ws.take((features, features), features)
    b = ws.take((features,), features)
    inits = [tensor("W", w), tensor("B", b), tensor("one", np.array([1.5], np.float32)), tensor("two", np.array([2.0], np.float32)),
             tensor("slope", (0.05 + 0.2 * np.abs(ws.take((features,), 1))).astype(np.float32)),
             tensor("lo", (-0.25 * np.ones((1, features))).astype(np.float32))]
    nodes = [node("Gemm", ["X", "W", "B"], ["H"]),
             node("Abs", ["H"], ["Hp0"]), node("Add", ["Hp0", "one"], ["Hpos"])]  # strictly positive branch input
    outs = []

    def br(op, src="H", attrs=()):
        o = f"o_{len(outs)}"
        nodes.append(node(op, [src], [o], list(attrs)))
        outs.append(o)

    for op in ("Exp", "Neg", "Abs", "Softplus", "HardSwish", "Erf", "Floor", "Ceil", "Softsign", "Round", "Sigmoid", "Tanh", "Relu"):
        br(op)
    br("Elu", attrs=[attr_f("alpha", 0.7)])
    br("Selu")
    br("HardSigmoid", attrs=[attr_f("alpha", 0.3), attr_f("beta", 0.4)])
    br("LeakyRelu", attrs=[attr_f("alpha", 0.2)])
    for op in ("Log", "Sqrt", "Reciprocal"):
        br(op, "Hpos")
    for op, rhs in (("Pow", "two"), ("Min", "lo"), ("Max", "lo"), ("PRelu", "slope")):
        o = f"o_{len(outs)}"
        nodes.append(node(op, ["H", rhs], [o]))
        outs.append(o)
    o = f"o_{len(outs)}"
    nodes.append(node("Max", ["lo", "H"], [o]))  # constant on the left
    outs.append(o)
    nodes.append(node("Concat", outs, ["Y"], [attr_i("axis", 1)]))
    return model("unary_zoo", nodes, inits, [value_info("X", ["N", features])], [value_info("Y", ["N", features * len(outs)])], opset=13)


def exporter_reshape(c: int = 8, hw: int = 6, classes: int = 5) -> bytes:
    """The PyTorch-exporter idiom `x.view(x.size(0), -1)`: Shape -> Gather(0) -> Unsqueeze -> Concat([n, -1]) -> Reshape,
    after a small conv + ReduceMean-free head, then Gemm + ArgMax with an INT64 output (label as f32 value)."""
    ws = _WeightStream(91)
    wc = ws.take((c, 3, 3, 3), 27)
    bc = ws.take((c,), 27)
    feat = c * hw * hw
    wf = ws.take((feat, classes), feat)
    bf = ws.take((classes,), feat)
    inits = [tensor("wc", wc), tensor("bc", bc), tensor("wf", wf), tensor("bf", bf), tensor("i0", np.array(0, np.int64).reshape(())),
             tensor("ax0", np.array([0], np.int64)), tensor("m1", np.array([-1], np.int64))]
    nodes = [node("Conv", ["X", "wc", "bc"], ["c1"], [attr_ints("kernel_shape", [3, 3]), attr_ints("pads", [1, 1, 1, 1])]),
             node("Relu", ["c1"], ["r1"]),
             node("Shape", ["r1"], ["shp"]),
             node("Gather", ["shp", "i0"], ["n"], [attr_i("axis", 0)]),
             node("Unsqueeze", ["n", "ax0"], ["n1"]),
             node("Concat", ["n1", "m1"], ["tgt"], [attr_i("axis", 0)]),
             node("Reshape", ["r1", "tgt"], ["flat"]),
             node("Gemm", ["flat", "wf", "bf"], ["logits"]),
             node("ArgMax", ["logits"], ["Y"], [attr_i("axis", 1), attr_i("keepdims", 1)])]
    return model("exporter_reshape", nodes, inits, [value_info("X", ["N", 3, hw, hw])], [value_info("Y", ["N", 1], INT64)], opset=13)


def concat_heads(features: int = 24) -> bytes:
    """Two dense towers over the same input, concatenated on the feature axis, then a head + Softmax."""
    ws = _WeightStream(55)
    inits, nodes = [], []
    for t, m in enumerate((12, 20)):
        w, b = ws.take((features, m), features), ws.take((m,), features)
        inits += [tensor(f"W{t}", w), tensor(f"B{t}", b)]
        nodes += [node("Gemm", ["X", f"W{t}", f"B{t}"], [f"h{t}"]), node("Tanh" if t else "Relu", [f"h{t}"], [f"a{t}"])]
    nodes.append(node("Concat", ["a0", "X", "a1"], ["cat"], [attr_i("axis", 1)]))
    k = 12 + features + 20
    w, b = ws.take((k, 7), k), ws.take((7,), k)
    inits += [tensor("Wh", w), tensor("Bh", b)]
    nodes += [node("Gemm", ["cat", "Wh", "Bh"], ["z"]), node("Softmax", ["z"], ["Y"], [attr_i("axis", 1)])]
    return model("concat_heads", nodes, inits, [value_info("X", ["N", features])], [value_info("Y", ["N", 7])], opset=13)


def mobilenet_v2(classes: int = 100, in_hw: int = 64, width_mult: float = 0.5, seed: int = 4321) -> bytes:
    """MobileNetV2 topology (the model family of the reference's blob test, test_advanced_features.test:46-63):
    3x3/2 stem, inverted residual blocks (1x1 expand + ReLU6, 3x3 DEPTHWISE + ReLU6, 1x1 linear project, residual Add
    when shapes match), 1x1 head, ReduceMean over the spatial axes, Gemm.  ReLU6 = Clip(0, 6) with tensor bounds;
    BatchNormalization after every conv (folded by the loader)."""
    ws = _WeightStream(seed)
    nodes, inits = [], [tensor("zero", np.array(0.0, np.float32).reshape(())), tensor("six", np.array(6.0, np.float32).reshape(()))]
    uid = [0]

    def fresh(p):
        uid[0] += 1
        return f"{p}{uid[0]}"

    def ch(v):
        return max(8, int(v * width_mult + 4) // 8 * 8)

    def conv_bn(x, cin, cout, k, stride, groups, relu6):
        w = ws.take((cout, cin // groups, k, k), (cin // groups) * k * k)
        wn, y = fresh("w"), fresh("c")
        inits.append(tensor(wn, w))
        nodes.append(node("Conv", [x, wn], [y], [attr_ints("kernel_shape", [k, k]), attr_ints("strides", [stride, stride]),
                                                 attr_ints("pads", [k // 2] * 4), attr_i("group", groups)]))
        names = [fresh("bn_s"), fresh("bn_b"), fresh("bn_m"), fresh("bn_v")]
        arrs = ((1.0 + 0.1 * ws.take((cout,), 1)), 0.1 * ws.take((cout,), 1), 0.1 * ws.take((cout,), 1), 1.0 + 0.5 * np.abs(ws.take((cout,), 1)))
        for nme, arr in zip(names, arrs):
            inits.append(tensor(nme, arr.astype(np.float32)))
        z = fresh("b")
        nodes.append(node("BatchNormalization", [y] + names, [z], [attr_f("epsilon", 1e-5)]))
        if relu6:
            r = fresh("r")
            nodes.append(node("Clip", [z, "zero", "six"], [r]))
            return r
        return z

    cin = ch(32)
    x = conv_bn("X", 3, cin, 3, 2, 1, True)
    for t, c, n, s in ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 2, 2), (6, 96, 1, 1)):
        cout = ch(c)
        for i in range(n):
            stride = s if i == 0 else 1
            hid = cin * t
            y = x
            if t != 1:
                y = conv_bn(y, cin, hid, 1, 1, 1, True)
            y = conv_bn(y, hid, hid, 3, stride, hid, True)  # depthwise
            y = conv_bn(y, hid, cout, 1, 1, 1, False)
            if stride == 1 and cin == cout:
                a = fresh("s")
                nodes.append(node("Add", [x, y], [a]))
                y = a
            x, cin = y, cout
    head = ch(640)
    x = conv_bn(x, cin, head, 1, 1, 1, True)
    g = fresh("g")
    nodes.append(node("ReduceMean", [x], [g], [attr_ints("axes", [2, 3]), attr_i("keepdims", 0)]))
    w, b = ws.take((head, classes), head), ws.take((classes,), head)
    inits += [tensor("fc_w", w), tensor("fc_b", b)]
    nodes.append(node("Gemm", [g, "fc_w", "fc_b"], ["Y"]))
    return model("mobilenet_v2", nodes, inits, [value_info("X", ["N", 3, in_hw, in_hw])], [value_info("Y", ["N", classes])], opset=13)


def se_net(c: int = 16, hw: int = 10, classes: int = 6) -> bytes:
    """Conv -> squeeze-and-excitation block (GlobalAveragePool -> 1x1 Conv -> Relu -> 1x1 Conv -> HardSigmoid ->
    Mul gate [N,C,1,1] over [N,C,H,W]) -> residual Add with a gated copy -> GAP -> Gemm.  MobileNetV3 / EfficientNet idiom."""
    ws = _WeightStream(31)
    inits, nodes = [], []

    def conv(x, cin, cout, k, out, act=None):
        w, b = ws.take((cout, cin, k, k), cin * k * k), ws.take((cout,), cin * k * k)
        inits.extend([tensor(out + "_w", w), tensor(out + "_b", b)])
        nodes.append(node("Conv", [x, out + "_w", out + "_b"], [out if act is None else out + "_pre"],
                          [attr_ints("kernel_shape", [k, k]), attr_ints("pads", [k // 2] * 4)]))
        if act:
            nodes.append(node(act, [out + "_pre"], [out]))
        return out

    x = conv("X", 4, c, 3, "stem", "Relu")
    sq = "sq"
    nodes.append(node("GlobalAveragePool", [x], [sq]))
    r = conv(sq, c, c // 4, 1, "se_r", "Relu")
    e = conv(r, c // 4, c, 1, "se_e", "HardSigmoid")
    nodes.append(node("Mul", [x, e], ["gated"]))
    nodes.append(node("Mul", [e, x], ["gated2"]))  # gate on the left: commutative form
    nodes.append(node("Add", ["gated", "gated2"], ["sum"]))
    nodes.append(node("GlobalAveragePool", ["sum"], ["g"]))
    nodes.append(node("Flatten", ["g"], ["f"], [attr_i("axis", 1)]))
    w, b = ws.take((c, classes), c), ws.take((classes,), c)
    inits += [tensor("fc_w", w), tensor("fc_b", b)]
    nodes.append(node("Gemm", ["f", "fc_w", "fc_b"], ["Y"]))
    return model("se_net", nodes, inits, [value_info("X", ["N", 4, hw, hw])], [value_info("Y", ["N", classes])], opset=14)


def zoo_ops_net(hw: int = 16, classes: int = 7) -> tuple[bytes, dict]:
    """One small network made of the operators the ONNX Model Zoo's vision models add to plain conv nets:
    LRN (AlexNet / GoogLeNet), explicit asymmetric Pad in front of a VALID Conv (TF / Keras exporters), channel Split,
    Concat and the Reshape -> Transpose -> Reshape channel shuffle (ShuffleNet), channel Slice, n-ary Sum and
    GlobalMaxPool.  Returns (model bytes, weights by name) so a test can restate it in numpy."""
    ws = _WeightStream(47)
    inits, nodes, wts = [], [], {}

    def conv(x, cin, cout, k, out, pads, stride=1, groups=1, act=None):
        w, b = ws.take((cout, cin // groups, k, k), (cin // groups) * k * k), ws.take((cout,), cin * k * k)
        wts[out] = (w, b)
        inits.extend([tensor(out + "_w", w), tensor(out + "_b", b)])
        nodes.append(node("Conv", [x, out + "_w", out + "_b"], [out if act is None else out + "_pre"],
                          [attr_ints("kernel_shape", [k, k]), attr_ints("pads", pads), attr_ints("strides", [stride, stride]),
                           attr_i("group", groups)]))
        if act:
            nodes.append(node(act, [out + "_pre"], [out]))
        return out

    conv("X", 3, 16, 3, "c1", [1, 1, 1, 1], act="Relu")
    nodes.append(node("LRN", ["c1"], ["n1"], [attr_i("size", 5), attr_f("alpha", 0.05), attr_f("beta", 0.75), attr_f("bias", 1.5)]))
    nodes.append(node("MaxPool", ["n1"], ["p1"], [attr_ints("kernel_shape", [2, 2]), attr_ints("strides", [2, 2])]))
    h1 = hw // 2
    inits.append(tensor("pads", np.array([0, 0, 0, 1, 0, 0, 2, 1], np.int64)))  # top 0, left 1, bottom 2, right 1
    nodes.append(node("Pad", ["p1", "pads"], ["pp"]))
    conv("pp", 16, 32, 3, "c2", [0, 0, 0, 0], stride=2, act="Relu")
    h2 = (h1 + 2 - 3) // 2 + 1
    nodes.append(node("Split", ["c2"], ["keep", "work"], [attr_i("axis", 1), attr_ints("split", [16, 16])]))
    conv("work", 16, 16, 1, "b1", [0, 0, 0, 0], act="Relu")
    conv("b1", 16, 16, 3, "b2", [1, 1, 1, 1], groups=16)
    conv("b2", 16, 16, 1, "b3", [0, 0, 0, 0], act="Relu")
    nodes.append(node("Concat", ["keep", "b3"], ["cat"], [attr_i("axis", 1)]))
    inits += [tensor("shape5", np.array([0, 2, 16, h2, h2], np.int64)), tensor("shape4", np.array([0, 32, h2, h2], np.int64))]
    nodes += [node("Reshape", ["cat", "shape5"], ["r5"]), node("Transpose", ["r5"], ["t5"], [attr_ints("perm", [0, 2, 1, 3, 4])]),
              node("Reshape", ["t5", "shape4"], ["shuf"])]
    inits += [tensor("s_st", np.array([8], np.int64)), tensor("s_en", np.array([24], np.int64)), tensor("s_ax", np.array([1], np.int64))]
    nodes.append(node("Slice", ["shuf", "s_st", "s_en", "s_ax"], ["mid"]))
    conv("mid", 16, 32, 1, "s1", [0, 0, 0, 0])
    conv("shuf", 32, 32, 1, "s2", [0, 0, 0, 0])
    nodes.append(node("Sum", ["s1", "s2", "shuf"], ["tot"]))
    nodes.append(node("GlobalMaxPool", ["tot"], ["g"]))
    nodes.append(node("Flatten", ["g"], ["f"], [attr_i("axis", 1)]))
    w, b = ws.take((32, classes), 32), ws.take((classes,), 32)
    wts["fc"] = (w, b)
    inits += [tensor("fc_w", w), tensor("fc_b", b)]
    nodes.append(node("Gemm", ["f", "fc_w", "fc_b"], ["Y"]))
    blob = model("zoo_ops", nodes, inits, [value_info("X", ["N", 3, hw, hw])], [value_info("Y", ["N", classes])], opset=13)
    return blob, wts


def write(path: str, blob: bytes) -> str:
    with open(path, "wb") as fh:
        fh.write(blob)
    return path


def sklearn_pipeline(features: int = 30, classes: int = 3, kind: str = "classifier", post: str = "SOFTMAX",
                     labels: Sequence[int] | None = None, normalizer: str | None = None, scaler: bool = True,
                     output: str = "label", seed: int = 99) -> bytes:
    """The graph skl2onnx writes for Pipeline(StandardScaler, LogisticRegression / LinearRegression): ai.onnx.ml
    Scaler -> LinearClassifier (label, scores) [-> Normalizer] or -> LinearRegressor.  `output` picks which value
    is graph output 0 -- the one the reference serves (engine.rs:146-149): "label" (int64 [N]), "scores" ([N,E])."""
    ws = _WeightStream(seed)
    nodes, x = [], "X"
    if scaler:
        off = ws.take((features,), 1)
        sc = (1.0 + 0.5 * ws.take((features,), 1)).astype(np.float32)
        nodes.append(node("Scaler", [x], ["Xs"], [attr_floats("offset", off), attr_floats("scale", sc)], domain=ML_DOMAIN))
        x = "Xs"
    coef = ws.take((classes, features), features)
    icpt = ws.take((classes,), features)
    if kind == "regressor":
        nodes.append(node("LinearRegressor", [x], ["Y"],
                          [attr_floats("coefficients", coef.ravel()), attr_floats("intercepts", icpt),
                           attr_i("targets", classes), attr_s("post_transform", post)], domain=ML_DOMAIN))
        outs = [value_info("Y", ["N", classes])]
    else:
        labels = list(labels) if labels is not None else list(range(classes))
        nodes.append(node("LinearClassifier", [x], ["label", "scores"],
                          [attr_floats("coefficients", coef.ravel()), attr_floats("intercepts", icpt),
                           attr_ints("classlabels_ints", labels), attr_s("post_transform", post)], domain=ML_DOMAIN))
        prob = "scores"
        if normalizer:
            nodes.append(node("Normalizer", ["scores"], ["probabilities"], [attr_s("norm", normalizer)], domain=ML_DOMAIN))
            prob = "probabilities"
        o_label, o_prob = value_info("label", ["N"], INT64), value_info(prob, ["N", classes])
        outs = [o_label, o_prob] if output == "label" else [o_prob, o_label]
    return model("sklearn_pipeline", nodes, [], [value_info("X", ["N", features])], outs, opset=13, ml_opset=1)


# ------------------------------------------------------------------------------------------
# ai.onnx.ml tree ensembles (TreeEnsembleRegressor / TreeEnsembleClassifier, opsets 1 and 3)
# ------------------------------------------------------------------------------------------

TREE_MODES = ("BRANCH_LEQ", "BRANCH_LT", "BRANCH_GTE", "BRANCH_GT", "BRANCH_EQ", "BRANCH_NEQ")
DOUBLE = 11


def tensor_f64(name: str, arr) -> bytes:
    """A DOUBLE TensorProto (raw_data): the *_as_tensor attributes of ai.onnx.ml opset 3."""
    a = np.asarray(arr, dtype=np.float64).ravel()
    return _vi(1, a.size) + _vi(2, DOUBLE) + _ld(9, a.astype("<f8").tobytes()) + _s(8, name)


def attr_tensor(name: str, t: bytes) -> bytes:
    return _s(1, name) + _ld(5, t) + _vi(20, 4)


def tree_ensemble_spec(features: int = 30, trees: int = 10, depth: int = 6, kind: str = "regressor", targets: int = 1,
                       labels: Sequence[int] | None = None, aggregate: str = "SUM", post: str = "NONE", ragged: bool = False,
                       modes: Sequence[str] = ("BRANCH_LEQ",), missing: bool = False, as_tensor: bool = False,
                       binary: str | None = None, base_values: bool = False, thresholds=None, pow2_leaves: bool = False,
                       seed: int = 7) -> dict:
    """Seeded tree ensemble as the attribute arrays an exporter writes.  Node ids are local to each tree and shuffled, and the
    node entries of all trees are interleaved.  ragged: trees of a random shape with one path of `depth` levels (forest-like);
    else full trees of `depth` levels (GBDT-like).  thresholds: a pool of values (e.g. values of the table) to draw from, else
    U(-1, 1).  as_tensor: thresholds, weights and base values as double tensors, each threshold moved by a quarter f32 ulp off
    its pool value (round-to-nearest would move it back and flip decisions).  binary: None, "signed" (GBDT/XGBoost log-odds
    leaves, some negative) or "positive" (weights >= 0, NONE only): the single-column classifier form with two classes.
    pow2_leaves: E = 1 leaves with distinct powers of two (every leaf choice readable from an exact sum; few leaves only)."""
    rng = np.random.default_rng(seed)
    cls = kind == "classifier"
    E = len(labels) if cls and labels is not None else (2 if cls and binary else (3 if cls else targets))
    labels = list(labels) if labels is not None else list(range(E))
    pool = None if thresholds is None else np.asarray(thresholds, dtype=np.float32).ravel()
    nodes = []  # (tree, id, feature, mode, value, true, false, missing)
    leaves = []  # (tree, id, class/target, weight)
    pow2 = 0
    for t in range(trees):
        shape = []  # per node: (depth, children or None)
        def grow(d, spine):
            i = len(shape)
            shape.append(None)
            split = d < depth and (not ragged or spine or (len(shape) < 4000 and rng.random() < (0.9 if d < 3 else 0.55)))
            if split:
                go_left = bool(rng.integers(2))
                a = grow(d + 1, spine and go_left)
                b = grow(d + 1, spine and not go_left)
                shape[i] = (a, b)
            return i
        grow(0, True)
        ids = rng.permutation(len(shape)) * 3 + 1  # local, shuffled, sparse
        tid = t * 2 + 5
        for i, ch in enumerate(shape):
            if ch is None:
                nodes.append((tid, int(ids[i]), 0, "LEAF", 0.0, 0, 0, 0))
                if pow2_leaves:
                    leaves.append((tid, int(ids[i]), 0, float(2.0 ** pow2)))
                    pow2 += 1
                    continue
                r = rng.random()
                if r < 0.08:
                    continue  # a leaf with no entry contributes 0
                if binary:
                    w = rng.normal(0, 0.5) if binary == "signed" else rng.uniform(0, 1.0 / trees)
                    leaves.append((tid, int(ids[i]), 1, float(w)))
                    continue
                for j in range(E):
                    w = rng.uniform(0, 1) if cls else rng.normal(0, 1)
                    leaves.append((tid, int(ids[i]), j, float(w)))
                if r > 0.9:  # a repeated entry for one target: summed
                    leaves.append((tid, int(ids[i]), int(rng.integers(E)), float(rng.normal(0, 0.5))))
                continue
            f = int(rng.integers(features))
            v = float(pool[rng.integers(pool.size)]) if pool is not None else float(np.float32(rng.uniform(-1, 1)))
            if as_tensor:
                sp = float(np.spacing(np.float32(abs(v)) if v != 0 else np.float32(1e-30)))
                v = v + (0.25 if rng.integers(2) else -0.25) * sp
            mode = str(modes[rng.integers(len(modes))])
            mv = int(rng.integers(2)) if missing else 0
            nodes.append((tid, int(ids[i]), f, mode, v, int(ids[ch[0]]), int(ids[ch[1]]), mv))
    order = rng.permutation(len(nodes))
    nodes = [nodes[i] for i in order]
    lorder = rng.permutation(len(leaves))
    leaves = [leaves[i] for i in lorder]
    spec = {
        "kind": kind, "features": features, "E": E, "labels": labels, "aggregate": aggregate, "post": post,
        "as_tensor": as_tensor, "missing": missing,
        "nodes_treeids": [n[0] for n in nodes], "nodes_nodeids": [n[1] for n in nodes], "nodes_featureids": [n[2] for n in nodes],
        "nodes_modes": [n[3] for n in nodes], "nodes_values": np.array([n[4] for n in nodes], dtype=np.float64),
        "nodes_truenodeids": [n[5] for n in nodes], "nodes_falsenodeids": [n[6] for n in nodes],
        "nodes_missing_value_tracks_true": [n[7] for n in nodes],
        "leaf_treeids": [l[0] for l in leaves], "leaf_nodeids": [l[1] for l in leaves], "leaf_ids": [l[2] for l in leaves],
        "leaf_weights": np.array([l[3] for l in leaves], dtype=np.float64),
        "base_values": None,
    }
    if not as_tensor:  # f32 attributes: the values ARE f32
        spec["nodes_values"] = spec["nodes_values"].astype(np.float32).astype(np.float64)
        spec["leaf_weights"] = spec["leaf_weights"].astype(np.float32).astype(np.float64)
    if base_values:
        spec["base_values"] = np.array(rng.normal(0, 0.5, 1 if binary else E), dtype=np.float32).astype(np.float64)
    return spec


def tree_ensemble_from_spec(spec: dict, scaler: tuple | None = None, output: str = "label", ml_opset: int | None = None) -> bytes:
    """The ONNX model of a tree_ensemble_spec() dict: [Scaler(offset, scale) ->] TreeEnsembleRegressor (output Y [N, E]) or
    TreeEnsembleClassifier (label int64 [N], probabilities [N, E]; `output` = which of the two is graph output 0)."""
    cls = spec["kind"] == "classifier"
    F = spec["features"]
    nodes, x = [], "X"
    if scaler is not None:
        nodes.append(node("Scaler", [x], ["Xs"], [attr_floats("offset", scaler[0]), attr_floats("scale", scaler[1])], domain=ML_DOMAIN))
        x = "Xs"
    nd, (o_first, o_second) = _tree_node(spec, x)
    nodes.append(nd)
    outs = ([o_first, o_second] if output == "label" else [o_second, o_first]) if cls else [o_first]
    return model("tree_ensemble", nodes, [], [value_info("X", ["N", F])], outs, opset=13,
                 ml_opset=ml_opset if ml_opset is not None else (3 if spec["as_tensor"] else 1))


def _tree_node(spec: dict, x: str, outputs: Sequence[str] = ("label", "probabilities")) -> tuple[bytes, tuple]:
    """The TreeEnsemble node of a tree_ensemble_spec() dict reading `x`, and the value infos of its (label, scores) outputs (regressor:
    (Y, None))."""
    cls = spec["kind"] == "classifier"
    E = spec["E"]
    at = bool(spec["as_tensor"])
    def floats(name, vals):
        return attr_tensor(name + "_as_tensor", tensor_f64("", vals)) if at else attr_floats(name, np.asarray(vals, dtype=np.float32))
    attrs = [attr_ints("nodes_treeids", spec["nodes_treeids"]), attr_ints("nodes_nodeids", spec["nodes_nodeids"]),
             attr_ints("nodes_featureids", spec["nodes_featureids"]), attr_strings("nodes_modes", spec["nodes_modes"]),
             floats("nodes_values", spec["nodes_values"]), attr_ints("nodes_truenodeids", spec["nodes_truenodeids"]),
             attr_ints("nodes_falsenodeids", spec["nodes_falsenodeids"]),
             attr_s("aggregate_function", spec["aggregate"]), attr_s("post_transform", spec["post"])]
    if spec["missing"]:
        attrs.append(attr_ints("nodes_missing_value_tracks_true", spec["nodes_missing_value_tracks_true"]))
    p = "class_" if cls else "target_"
    attrs += [attr_ints(p + "treeids", spec["leaf_treeids"]), attr_ints(p + "nodeids", spec["leaf_nodeids"]),
              attr_ints(p + "ids", spec["leaf_ids"]), floats(p + "weights", spec["leaf_weights"])]
    if spec["base_values"] is not None:
        attrs.append(floats("base_values", spec["base_values"]))
    if cls:
        attrs.append(attr_ints("classlabels_int64s", spec["labels"]))
        nd = node("TreeEnsembleClassifier", [x], list(outputs), attrs, domain=ML_DOMAIN)
        return nd, (value_info(outputs[0], ["N"], INT64), value_info(outputs[1], ["N", E]))
    attrs.append(attr_i("n_targets", E))
    return node("TreeEnsembleRegressor", [x], ["Y"], attrs, domain=ML_DOMAIN), (value_info("Y", ["N", E]), None)


def tree_ensemble(scaler: tuple | None = None, output: str = "label", **kw) -> bytes:
    """Seeded TreeEnsembleRegressor / TreeEnsembleClassifier model (keywords: tree_ensemble_spec)."""
    return tree_ensemble_from_spec(tree_ensemble_spec(**kw), scaler=scaler, output=output)


# ------------------------------------------------------------------------------------------
# ai.onnx.ml support-vector machines (SVMRegressor / SVMClassifier)
# ------------------------------------------------------------------------------------------

SVM_KERNELS = ("LINEAR", "POLY", "RBF", "SIGMOID")


def svm_spec(features: int = 30, n_sv: int = 256, kind: str = "classifier", classes: int = 3, kernel: str = "RBF",
             probabilities: bool = False, post: str = "NONE", per_class: Sequence[int] | None = None,
             labels: Sequence[int] | None = None, gamma: float | None = None, coef0: float = 0.5, degree: int = 3,
             offset: float = 0.0, seed: int = 7) -> dict:
    """Seeded SVM as the attribute arrays an exporter writes (libsvm's one-vs-one layout for the classifier).  kind: "regressor",
    "one_class" or "classifier".  per_class: SVs per class block (default: n_sv spread unevenly over the classes).  Support vectors
    are offset + N(0, 1) in f32; gamma defaults to 1 / features.  Every value is f32, as the attributes store it."""
    rng = np.random.default_rng(seed)
    cls = kind == "classifier"
    C = classes if cls else 1
    if cls and per_class is None:
        w = rng.uniform(0.5, 1.5, C)
        per_class = np.maximum(1, np.floor(w / w.sum() * n_sv)).astype(int)
        per_class[-1] = max(1, n_sv - int(per_class[:-1].sum()))
    per_class = [int(v) for v in per_class] if cls else [n_sv]
    n_sv = int(sum(per_class))
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    g = float(np.float32(1.0 / features if gamma is None else gamma))
    Q = C - 1 if cls else 1
    P = C * (C - 1) // 2 if cls else 1
    spec = {
        "kind": kind, "features": features, "kernel": kernel, "post": post, "classes": C,
        "labels": list(labels) if labels is not None else list(range(C)),
        "vectors_per_class": per_class, "n_sv": n_sv,
        "support_vectors": f32(offset + rng.normal(0, 1, (n_sv, features))),
        "coefficients": f32(rng.normal(0, 1, (Q, n_sv))),
        "rho": f32(rng.normal(0, 0.5, P)),
        "kernel_params": f32([g, coef0, degree]),
        "prob_a": f32(-rng.uniform(0.5, 2.0, P)) if (cls and probabilities) else None,
        "prob_b": f32(rng.normal(0, 0.2, P)) if (cls and probabilities) else None,
    }
    if kind == "one_class":
        spec["coefficients"] = f32(np.abs(spec["coefficients"]))
    return spec


def svm_from_spec(spec: dict, scaler: tuple | None = None, output: str = "label") -> bytes:
    """The ONNX model of an svm_spec() dict (or of the same keys taken from a fitted estimator): [Scaler(offset, scale) ->]
    SVMRegressor (output Y [N, 1]) or SVMClassifier (label int64 [N], probabilities [N, *]; `output` = which is graph output 0)."""
    cls = spec["kind"] == "classifier"
    F = spec["features"]
    nodes, x = [], "X"
    if scaler is not None:
        nodes.append(node("Scaler", [x], ["Xs"], [attr_floats("offset", scaler[0]), attr_floats("scale", scaler[1])], domain=ML_DOMAIN))
        x = "Xs"
    nd, (o_first, o_second) = _svm_node(spec, x)
    nodes.append(nd)
    outs = ([o_first, o_second] if output == "label" else [o_second, o_first]) if cls else [o_first]
    return model("svm", nodes, [], [value_info("X", ["N", F])], outs, opset=13, ml_opset=1)


def _svm_node(spec: dict, x: str, outputs: Sequence[str] = ("label", "probabilities")) -> tuple[bytes, tuple]:
    """The SVM node of an svm_spec() dict reading `x`, and the value infos of its (label, scores) outputs (regressor: (Y, None))."""
    cls = spec["kind"] == "classifier"
    attrs = [attr_s("kernel_type", spec["kernel"]), attr_floats("kernel_params", spec["kernel_params"]),
             attr_floats("support_vectors", np.asarray(spec["support_vectors"], dtype=np.float32).ravel()),
             attr_floats("coefficients", np.asarray(spec["coefficients"], dtype=np.float32).ravel()),
             attr_floats("rho", np.asarray(spec["rho"], dtype=np.float32).ravel()), attr_s("post_transform", spec["post"])]
    if cls:
        attrs += [attr_ints("vectors_per_class", spec["vectors_per_class"]), attr_ints("classlabels_ints", spec["labels"])]
        if spec.get("prob_a") is not None:
            attrs += [attr_floats("prob_a", spec["prob_a"]), attr_floats("prob_b", spec["prob_b"])]
        C = spec["classes"]
        cols = C if spec.get("prob_a") is not None else (2 if C == 2 else C * (C - 1) // 2)
        nd = node("SVMClassifier", [x], list(outputs), attrs, domain=ML_DOMAIN)
        return nd, (value_info(outputs[0], ["N"], INT64), value_info(outputs[1], ["N", cols]))
    attrs += [attr_i("n_supports", spec["n_sv"]), attr_i("one_class", 1 if spec["kind"] == "one_class" else 0)]
    return node("SVMRegressor", [x], ["Y"], attrs, domain=ML_DOMAIN), (value_info("Y", ["N", 1]), None)


def svm(scaler: tuple | None = None, output: str = "label", **kw) -> bytes:
    """Seeded SVMRegressor / SVMClassifier model (keywords: svm_spec)."""
    return svm_from_spec(svm_spec(**kw), scaler=scaler, output=output)


# ------------------------------------------------------------------------------------------
# recurrent layers (LSTM, GRU, RNN) in the forms exporters write them
# ------------------------------------------------------------------------------------------

_RNN_GATES = {"LSTM": 4, "GRU": 3, "RNN": 1}


def recurrent_spec(op: str = "LSTM", T: int = 24, F: int = 8, H: int = 64, layers: int = 1, direction: str = "forward",
                   linear_before_reset: int = 1, activation: str = "Tanh", initial: float = 0.0, bias: bool = True,
                   r_scale: float = 1.0, seed: int = 11) -> dict:
    """Seeded stack of ONNX recurrent layers: per layer W [D, G*H, F_in], R [D, G*H, H], B [D, 2*G*H] in ONNX gate order (LSTM i,o,f,c;
    GRU z,r,h), U(+-1/sqrt(H)) like PyTorch.  initial != 0: a constant initial state N(0, initial) per layer (h0, and c0 for LSTM), one
    row [D, H].  r_scale scales R (Relu RNNs: keep its spectral norm below 1)."""
    rng = np.random.default_rng(seed)
    G, D = _RNN_GATES[op], 2 if direction == "bidirectional" else 1
    k = 1.0 / np.sqrt(H)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    ls = []
    for i in range(layers):
        fin = F if i == 0 else D * H
        ls.append({"W": f32(rng.uniform(-k, k, (D, G * H, fin))), "R": f32(rng.uniform(-k, k, (D, G * H, H)) * r_scale),
                   "B": f32(rng.uniform(-k, k, (D, 2 * G * H))) if bias else None,
                   "h0": f32(rng.normal(0, initial, (D, H))) if initial else None,
                   "c0": f32(rng.normal(0, initial, (D, H))) if initial and op == "LSTM" else None})
    return {"op": op, "T": T, "F": F, "H": H, "D": D, "direction": direction, "linear_before_reset": linear_before_reset,
            "activation": activation, "layers": ls}


def torch_recurrent_spec(module) -> dict:
    """The recurrent_spec() dict of a torch.nn.LSTM / GRU / RNN (any num_layers, bidirectional or not).  PyTorch stores the gates as
    i,f,g,o (LSTM) and r,z,n (GRU); ONNX wants i,o,f,c and z,r,h: the permutation lives here.  GRU: linear_before_reset = 1."""
    op = type(module).__name__
    H, D = module.hidden_size, 2 if module.bidirectional else 1
    order = {"LSTM": [0, 3, 1, 2], "GRU": [1, 0, 2], "RNN": [0]}[op]

    def gates(a):
        a = a.detach().cpu().numpy().astype(np.float32)
        return np.concatenate([a[g * H:(g + 1) * H] for g in order], axis=0)

    ls = []
    for i in range(module.num_layers):
        sfx = [f"_l{i}", f"_l{i}_reverse"][:D]
        W = np.stack([gates(getattr(module, "weight_ih" + x)) for x in sfx])
        R = np.stack([gates(getattr(module, "weight_hh" + x)) for x in sfx])
        B = np.stack([np.concatenate([gates(getattr(module, "bias_ih" + x)), gates(getattr(module, "bias_hh" + x))]) for x in sfx]) if module.bias else None
        ls.append({"W": W, "R": R, "B": B, "h0": None, "c0": None})
    act = "Relu" if op == "RNN" and module.nonlinearity == "relu" else "Tanh"
    return {"op": op, "T": None, "F": module.input_size, "H": H, "D": D, "direction": "bidirectional" if D == 2 else "forward",
            "linear_before_reset": 1, "activation": act, "layers": ls}


def recurrent_from_spec(spec: dict, T: int | None = None, form: str = "batch_first", tail: str = "seq", flat: bool = False,
                        head: tuple | None = None, scaler: tuple | None = None, initial: str = "const", opset: int = 14,
                        extra_attrs: Sequence[bytes] = (), last_index: int = -1, state_outputs: bool = False,
                        seq_lens: dict | None = None) -> bytes:
    """The ONNX model of a recurrent_spec() / torch_recurrent_spec() dict, input X [N, T, F] (flat: [N, T*F] -> Reshape).
    form: "batch_first" (Transpose(1,0,2) -> time-major layers -> Transpose back, what PyTorch writes for batch_first=True) or "layout1"
    (layout = 1, no Transpose).  Layers are stacked through Squeeze(axes 1) (one direction) or Transpose(0,2,1,3) + Reshape [0,0,-1].
    tail: "seq" -> Y [N, T, D*H]; "last_gather" / "last_slice" -> step `last_index` of it [N, D*H]; "y_h" / "y_c" -> the last layer's final
    state [N, D*H] (Squeeze(axes 0) for one direction, Transpose(1,0,2) + Reshape for two).  head = (W [D*H, M], b [M], act or None): a Gemm
    (+ activation) behind a 2-D tail.  scaler = (offset, scale) over the flat T*F columns (needs flat).  initial: how a layer's constant initial
    state is written: "const" ([D, 1, H] initializer), "expand" (Shape(X) -> Gather -> Unsqueeze -> Concat -> Expand) or "fill" (the
    same shape sub-graph -> ConstantOfShape: a state of one value, as PyTorch writes its zeros).  state_outputs: the
    last layer's Y_h (and Y_c) are graph outputs too, under the names "Y_h" / "Y_c".
    seq_lens (None: no input 4, the bytes of every model so far): per-row sequence lengths as input 4 of EVERY layer; X is then flat
    ([N, T*F]).  A dict with "form": where the lengths come from: "rank1" (one more input len [N]), "col" (len [N, 1]), "wide" (meta [N, k],
    column "col" of it) or "single" (no second input: X is [N, T*F + 1], the readings are Slice(X, 0:T*F) and the length is its last column);
    "type": INT32 / INT64 / FLOAT (/ FLOAT16, single) of that input (default INT64; single: FLOAT); "cast": Cast(to = INT32) behind it
    (default: unless the type is INT32, as PyTorch writes Cast(lengths, INT32)); "squeeze": how [N, 1] becomes [N]: "squeeze"
    (Squeeze(axes = [1])), "reshape" (Reshape([-1])) or "flatten" (Flatten -> Squeeze); "pick" (wide): "slice" (Slice on axis 1, then the
    squeeze) or "gather" (Gather(axis = 1) by a scalar index: [N] at once).  Forms that are refused: "source": "transpose" (an [N, 1] input
    transposed to [1, N] and reshaped), "reduce_sum" (ReduceSum of an [N, T] mask), "activation" (ArgMax over X), "two_cols" (an [N, 2]
    input as it is); "shared": True (needs a 2-D tail: the length also multiplies the served output).  "extra_output": True adds the
    length as a second graph output "len_out", which is not the served one."""
    op, H, D, F = spec["op"], spec["H"], spec["D"], spec["F"]
    T = spec["T"] if T is None else T
    nodes, inits = [], []
    i64 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.int64)))  # noqa: E731
    x = "X"
    lens_value, lens_input, sl = "", None, None
    if seq_lens is not None:
        flat = True
        sl = dict(form="rank1", squeeze="squeeze", pick="slice", k=3, col=1, source="input", shared=False, extra_output=False)
        sl.update(seq_lens)
        sl.setdefault("type", FLOAT if sl["form"] == "single" else INT64)
        cast = sl.get("cast", sl["type"] != INT32)
        i64("sl_ax1", [1])
        v, shape1 = "len", False  # shape1: v is [N] already
        if sl["source"] == "transpose":
            lens_input = value_info("len", ["N", 1], sl["type"])
            nodes.append(node("Transpose", ["len"], ["len_t"], [attr_ints("perm", [1, 0])], name="sl_transpose"))
            v, sl["squeeze"] = "len_t", "reshape"
        elif sl["source"] == "reduce_sum":
            lens_input = value_info("len", ["N", T], sl["type"])
            nodes.append(node("ReduceSum", ["len", "sl_ax1"], ["len_s"], [attr_i("keepdims", 0)], name="sl_sum"))
            v, shape1 = "len_s", True
        elif sl["source"] == "activation":
            lens_input = value_info("len", ["N", 1], sl["type"])  # (declared and not read)
            nodes.append(node("ArgMax", ["X"], ["len_a"], [attr_i("axis", 1), attr_i("keepdims", 0)], name="sl_argmax"))
            v, shape1, cast = "len_a", True, True
        elif sl["source"] == "two_cols":
            lens_input = value_info("len", ["N", 2], sl["type"])
            shape1 = True
        elif sl["form"] == "rank1":
            lens_input = value_info("len", ["N"], sl["type"])
            shape1 = True
        elif sl["form"] == "col":
            lens_input = value_info("len", ["N", 1], sl["type"])
        elif sl["form"] == "single":
            i64("sl_x0", [0]); i64("sl_x1", [T * F]); i64("sl_c1", [T * F + 1])  # noqa: E702
            nodes += [node("Slice", ["X", "sl_x0", "sl_x1", "sl_ax1"], ["X_readings"], name="sl_readings"),
                      node("Slice", ["X", "sl_x1", "sl_c1", "sl_ax1"], ["len_c"], name="sl_slice")]
            x, v = "X_readings", "len_c"
        else:
            lens_input = value_info("meta", ["N", sl["k"]], sl["type"])
            v = "meta"
            if sl["pick"] == "gather":
                i64("sl_ix", sl["col"])
                nodes.append(node("Gather", [v, "sl_ix"], ["len_g"], [attr_i("axis", 1)], name="sl_gather"))
                v, shape1 = "len_g", True
            else:
                i64("sl_c0", [sl["col"]]); i64("sl_c1", [sl["col"] + 1])  # noqa: E702
                nodes.append(node("Slice", [v, "sl_c0", "sl_c1", "sl_ax1"], ["len_c"], name="sl_slice"))
                v = "len_c"
        if not shape1:
            if sl["squeeze"] == "reshape":
                i64("sl_flat", [-1])
                nodes.append(node("Reshape", [v, "sl_flat"], ["len_1"], name="sl_reshape"))
            else:
                if sl["squeeze"] == "flatten":
                    nodes.append(node("Flatten", [v], ["len_f"], [attr_i("axis", 1)], name="sl_flatten"))
                    v = "len_f"
                nodes.append(node("Squeeze", [v, "sl_ax1"], ["len_1"], name="sl_squeeze"))
            v = "len_1"
        if cast:
            nodes.append(node("Cast", [v], ["len_i32"], [attr_i("to", INT32)], name="sl_cast"))
            v = "len_i32"
        lens_value = v
    if scaler is not None:
        nodes.append(node("Scaler", [x], ["Xs"], [attr_floats("offset", scaler[0]), attr_floats("scale", scaler[1])], domain=ML_DOMAIN))
        x = "Xs"
    if flat:
        i64("flat_shape", [-1, T, F])
        nodes.append(node("Reshape", [x, "flat_shape"], ["X3"]))
        x = "X3"
    lay1 = form == "layout1"
    if not lay1:
        nodes.append(node("Transpose", [x], ["Xt"], [attr_ints("perm", [1, 0, 2])]))
        x = "Xt"
    i64("ax0", [0]); i64("ax1", [1]); i64("merge", [0, 0, -1])  # noqa: E702
    yh = yc = None
    for i, L in enumerate(spec["layers"]):
        p = f"l{i}_"
        inits += [tensor(p + "W", L["W"]), tensor(p + "R", L["R"])]
        ins = [x, p + "W", p + "R", "", lens_value, "", ""]
        if L["B"] is not None:
            inits.append(tensor(p + "B", L["B"]))
            ins[3] = p + "B"
        for slot, key in ((5, "h0"), (6, "c0")):
            if L.get(key) is None:
                continue
            v = L[key].reshape(1, D, H) if lay1 else L[key].reshape(D, 1, H)
            inits.append(tensor(p + key, v))
            ins[slot] = p + key
            if initial == "expand":  # broadcast over the row count of X, as exporters spell it
                i64(p + key + "_d", [D]); i64(p + key + "_h", [H]); i64(p + key + "_i", 0 if lay1 else 1)  # noqa: E702
                pieces = [p + key + "_n", p + key + "_d", p + key + "_h"] if lay1 else [p + key + "_d", p + key + "_n", p + key + "_h"]
                nodes += [node("Shape", [x], [p + key + "_s"]), node("Gather", [p + key + "_s", p + key + "_i"], [p + key + "_g"], [attr_i("axis", 0)]),
                          node("Unsqueeze", [p + key + "_g", "ax0"], [p + key + "_n"]), node("Concat", pieces, [p + key + "_shape"], [attr_i("axis", 0)]),
                          node("Expand", [p + key, p + key + "_shape"], [p + key + "_x"])]
                ins[slot] = p + key + "_x"
            elif initial == "fill":  # one value for the whole state (PyTorch's zeros): ConstantOfShape over the same shape sub-graph
                fill = np.asarray(L[key], dtype=np.float32).ravel()
                if not np.all(fill == fill[0]):
                    raise ValueError("initial='fill' needs a state of one value")
                i64(p + key + "_d", [D]); i64(p + key + "_h", [H]); i64(p + key + "_i", 0 if lay1 else 1)  # noqa: E702
                pieces = [p + key + "_n", p + key + "_d", p + key + "_h"] if lay1 else [p + key + "_d", p + key + "_n", p + key + "_h"]
                nodes += [node("Shape", [x], [p + key + "_s"]), node("Gather", [p + key + "_s", p + key + "_i"], [p + key + "_g"], [attr_i("axis", 0)]),
                          node("Unsqueeze", [p + key + "_g", "ax0"], [p + key + "_n"]), node("Concat", pieces, [p + key + "_shape"], [attr_i("axis", 0)]),
                          node("ConstantOfShape", [p + key + "_shape"], [p + key + "_x"], [attr_tensor("value", tensor("", fill[:1]))])]
                ins[slot] = p + key + "_x"
        while ins and ins[-1] == "":
            ins.pop()
        attrs = [attr_i("hidden_size", H), attr_s("direction", spec["direction"])] + list(extra_attrs)
        if lay1:
            attrs.append(attr_i("layout", 1))
        if op == "GRU":
            attrs.append(attr_i("linear_before_reset", spec["linear_before_reset"]))
        if op == "RNN" and spec["activation"] != "Tanh":
            attrs.append(attr_strings("activations", [spec["activation"]] * D))
        yh, yc = p + "Yh", p + "Yc"
        nodes.append(node(op, ins, [p + "Y", yh] + ([yc] if op == "LSTM" else []), attrs, name=f"rnn{i}"))
        if lay1:  # [N, T, D, H] -> [N, T, D*H]
            nodes.append(node("Reshape", [p + "Y", "merge"], [p + "S"]))
        elif D == 1:  # [T, 1, N, H] -> [T, N, H]
            nodes.append(node("Squeeze", [p + "Y", "ax1"], [p + "S"]))
        else:  # [T, 2, N, H] -> [T, N, 2, H] -> [T, N, 2H]
            nodes += [node("Transpose", [p + "Y"], [p + "Yt"], [attr_ints("perm", [0, 2, 1, 3])]), node("Reshape", [p + "Yt", "merge"], [p + "S"])]
        x = p + "S"
    C = D * H
    if tail in ("y_h", "y_c"):
        st = yh if tail == "y_h" else yc
        i64("flat2", [-1, C])
        if lay1:
            nodes.append(node("Reshape", [st, "flat2"], ["out2"]))
        elif D == 1:
            nodes.append(node("Squeeze", [st, "ax0"], ["out2"]))
        else:
            nodes += [node("Transpose", [st], ["st_t"], [attr_ints("perm", [1, 0, 2])]), node("Reshape", ["st_t", "flat2"], ["out2"])]
        out, dims = "out2", ["N", C]
    else:
        if not lay1:
            nodes.append(node("Transpose", [x], ["seq"], [attr_ints("perm", [1, 0, 2])]))
            x = "seq"
        out, dims = x, ["N", T, C]
        if tail == "last_gather":
            i64("last", last_index)
            nodes.append(node("Gather", [x, "last"], ["out2"], [attr_i("axis", 1)]))
            out, dims = "out2", ["N", C]
        elif tail == "last_slice":
            b = last_index % T
            i64("sl_b", [b]); i64("sl_e", [b + 1])  # noqa: E702
            nodes += [node("Slice", [x, "sl_b", "sl_e", "ax1"], ["sl"]), node("Squeeze", ["sl", "ax1"], ["out2"])]
            out, dims = "out2", ["N", C]
    if head is not None:
        Wd, bd, act = head
        inits += [tensor("head_W", np.asarray(Wd, dtype=np.float32)), tensor("head_b", np.asarray(bd, dtype=np.float32))]
        nodes.append(node("Gemm", [out, "head_W", "head_b"], ["score"]))
        out, dims = "score", ["N", int(np.asarray(Wd).shape[1])]
        if act:
            nodes.append(node(act, [out], ["prob"]))
            out = "prob"
    in_dims = ["N", T * F] if (flat or scaler is not None) else ["N", T, F]
    x_type = FLOAT
    if sl is not None:
        if sl["form"] == "single":
            in_dims, x_type = ["N", T * F + 1], sl["type"]
        if sl["shared"]:  # the length reaches the served output a second way
            nodes += [node("Cast", [lens_value], ["len_f32"], [attr_i("to", FLOAT)], name="sl_share_cast"),
                      node("Unsqueeze", ["len_f32", "sl_ax1"], ["len_f32c"], name="sl_share_col"), node("Mul", [out, "len_f32c"], ["out_scaled"], name="sl_share")]
            out = "out_scaled"
    outs = [value_info(out, dims)]
    if sl is not None and sl["extra_output"]:
        nodes.append(node("Cast", [lens_value], ["len_out"], [attr_i("to", INT64)], name="sl_out"))
        outs.append(value_info("len_out", ["N"], INT64))
    if state_outputs:
        sdims = ["N", D, H] if lay1 else [D, "N", H]
        nodes.append(node("Identity", [yh], ["Y_h"]))
        outs.append(value_info("Y_h", sdims))
        if op == "LSTM":
            nodes.append(node("Identity", [yc], ["Y_c"]))
            outs.append(value_info("Y_c", sdims))
    ins_info = [value_info("X", in_dims, x_type)] + ([lens_input] if lens_input is not None else [])
    return model("recurrent", nodes, inits, ins_info, outs, opset=opset, ml_opset=1 if scaler is not None else None)


# ------------------------------------------------------------------------------------------
# Transformer encoders (window Dense, LayerNormalization, self-attention, mean over time)
# ------------------------------------------------------------------------------------------

def transformer_spec(T: int = 24, F: int = 8, E: int = 64, h: int = 4, ff: int = 256, layers: int = 2, norm_first: bool = False,
                     act: str = "Relu", outputs: int = 1, causal: bool = False, final_norm: bool | None = None, eps: float = 1e-5,
                     weight_scale: float = 1.0, seed: int = 21) -> dict:
    """Seeded Transformer encoder: input projection F -> E, positional constant [T, E], `layers` encoder layers (self-attention with h heads,
    feed-forward E -> ff -> E, LayerNorm and residuals; norm_first: pre-norm), optional final LayerNorm (default: with norm_first), head
    E -> outputs.  All matrices are [in, out]; U(+-1/sqrt(fan_in)) like PyTorch's Linear, scaled by weight_scale."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731

    def lin(i, o):
        k = weight_scale / np.sqrt(i)
        return f32(rng.uniform(-k, k, (i, o))), f32(rng.uniform(-k, k, (o,)))

    def ln():
        return f32(1.0 + 0.1 * rng.standard_normal(E)), f32(0.1 * rng.standard_normal(E))

    ls = []
    for _ in range(layers):
        L = {}
        for nm, (i, o) in (("q", (E, E)), ("k", (E, E)), ("v", (E, E)), ("o", (E, E)), ("1", (E, ff)), ("2", (ff, E))):
            L["W" + nm], L["b" + nm] = lin(i, o)
        L["g1"], L["be1"] = ln()
        L["g2"], L["be2"] = ln()
        ls.append(L)
    Win, bin_ = lin(F, E)
    Wh, bh = lin(E, outputs)
    if final_norm is None:
        final_norm = norm_first
    return {"T": T, "F": F, "E": E, "h": h, "ff": ff, "norm_first": norm_first, "act": act, "eps": eps, "causal": causal, "layers": ls,
            "Win": Win, "bin": bin_, "pos": f32(0.5 * rng.standard_normal((T, E))), "final_norm": ln() if final_norm else None,
            "head_W": Wh, "head_b": bh}


def from_torch_encoder(encoder, T: int, head=None, causal: bool = False) -> dict:
    """The transformer_spec() dict of a torch.nn.TransformerEncoder(batch_first=True): in_proj_weight [3E, E] is split into Wq, Wk, Wv and
    every Linear transposed to [in, out].  No input projection and no positional constant (F = E); head: a torch.nn.Linear or None."""
    sd = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in encoder.state_dict().items()}
    l0 = encoder.layers[0]
    E, h, ff = l0.self_attn.embed_dim, l0.self_attn.num_heads, l0.linear1.out_features
    act = "Gelu" if "gelu" in getattr(l0.activation, "__name__", type(l0.activation).__name__).lower() else "Relu"
    ls = []
    for i in range(len(encoder.layers)):
        p = f"layers.{i}."
        W, b = sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"]
        L = {"Wq": W[:E].T.copy(), "Wk": W[E:2 * E].T.copy(), "Wv": W[2 * E:].T.copy(), "bq": b[:E].copy(), "bk": b[E:2 * E].copy(), "bv": b[2 * E:].copy(),
             "Wo": sd[p + "self_attn.out_proj.weight"].T.copy(), "bo": sd[p + "self_attn.out_proj.bias"],
             "W1": sd[p + "linear1.weight"].T.copy(), "b1": sd[p + "linear1.bias"], "W2": sd[p + "linear2.weight"].T.copy(), "b2": sd[p + "linear2.bias"],
             "g1": sd[p + "norm1.weight"], "be1": sd[p + "norm1.bias"], "g2": sd[p + "norm2.weight"], "be2": sd[p + "norm2.bias"]}
        ls.append(L)
    fin = (sd["norm.weight"], sd["norm.bias"]) if "norm.weight" in sd else None
    spec = {"T": T, "F": E, "E": E, "h": h, "ff": ff, "norm_first": bool(l0.norm_first), "act": act, "eps": float(l0.norm1.eps), "causal": causal,
            "layers": ls, "Win": None, "bin": None, "pos": None, "final_norm": fin, "head_W": None, "head_b": None}
    if head is not None:
        spec["head_W"] = head.weight.detach().cpu().numpy().astype(np.float32).T.copy()
        spec["head_b"] = head.bias.detach().cpu().numpy().astype(np.float32)
    return spec


def attention_nodes(nodes: list, inits: list, p: str, q: str, k: str, v: str, x_for_shape: str, T: int, E: int, h: int, scale: str = "scores_div",
                    k_transpose: str = "direct", mask=None, shape: str = "const", scale_value: float | None = None, softmax_axis: int = -1,
                    mask_left: bool = False, row_mask: dict | None = None, rotary=None) -> str:
    """Appends the batch-first self-attention sub-graph over q, k, v [N, T, E] (names) and returns the name of its [N, T, E] result.
    scale: "scores_div" (Div by sqrt(dh)), "scores_mul", "q" (Mul of Q) or "sqrt_both" (Q and K^T by sqrt(scale) each, what
    scaled_dot_product_attention exports); k_transpose: "direct" (0,2,3,1) or "two_step" ((0,2,1,3) then (0,1,3,2)); mask: None or an f32
    array added to the scores (mask_left: as the Add's first operand); shape: "const" targets or the exporter's Shape -> Gather -> Unsqueeze -> Concat sub-graph.
    row_mask: None or a per-row key mask, dict(src=<name of an [N, T] value>, form="add" | "replace", fill=<negative float>, from_ids=None | pad_id,
    unsqueeze="one" | "two" | "reshape", expand="none" | "const" | "shape", value=None | <what row_mask_value() returned>); see row_mask_value and
    row_mask_on_scores (mask_left: the mask term as the Add's first operand).
    rotary: None, True or the options of rotary_options(): a rotary embedding on the head-major Q and K (K: in front of the second Transpose of
    k_transpose "two_step", the only place where K is [N, h, T, dh])."""
    dh = E // h
    rot = rotary_options(rotary)
    assert rot is None or k_transpose == "two_step", "rotary needs K as [N, h, T, dh]: k_transpose='two_step'"
    sv = (1.0 / math.sqrt(dh)) if scale_value is None else scale_value
    i64 = lambda name, val: inits.append(tensor(name, np.asarray(val, dtype=np.int64)))  # noqa: E731
    f32 = lambda name, val: inits.append(tensor(name, np.asarray(val, dtype=np.float32)))  # noqa: E731
    if shape == "const":
        i64(p + "split", [0, T, h, dh])
        i64(p + "merge", [0, T, E])
        split_shape = merge_shape = None
    else:
        i64(p + "i0", 0); i64(p + "ax0", [0]); i64(p + "thd", [T, h, dh]); i64(p + "te", [T, E])  # noqa: E702
        nodes += [node("Shape", [x_for_shape], [p + "shp"]), node("Gather", [p + "shp", p + "i0"], [p + "n"], [attr_i("axis", 0)]),
                  node("Unsqueeze", [p + "n", p + "ax0"], [p + "n1"]),
                  node("Concat", [p + "n1", p + "thd"], [p + "split"], [attr_i("axis", 0)]),
                  node("Concat", [p + "n1", p + "te"], [p + "merge"], [attr_i("axis", 0)])]
    heads = {}
    for nm, src in (("q", q), ("k", k), ("v", v)):
        nodes.append(node("Reshape", [src, p + "split"], [p + nm + "4"], name=p + "split_" + nm))
        if nm == "k" and k_transpose == "direct":
            nodes.append(node("Transpose", [p + "k4"], [p + "kh"], [attr_ints("perm", [0, 2, 3, 1])], name=p + "tr_k"))
        elif nm == "k":
            nodes.append(node("Transpose", [p + "k4"], [p + "kh0"], [attr_ints("perm", [0, 2, 1, 3])], name=p + "tr_k0"))
            kh0 = p + "kh0" if rot is None or "k" not in rot["on"] else rotary_nodes(nodes, inits, p + "k_", p + "kh0", T, dh, rot)
            nodes.append(node("Transpose", [kh0], [p + "kh"], [attr_ints("perm", [0, 1, 3, 2])], name=p + "tr_k"))
        else:
            nodes.append(node("Transpose", [p + nm + "4"], [p + nm + "h"], [attr_ints("perm", [0, 2, 1, 3])], name=p + "tr_" + nm))
        heads[nm] = p + nm + "h"
        if rot is not None and nm != "k" and nm in rot["on"]:
            heads[nm] = rotary_nodes(nodes, inits, p + nm + "_", heads[nm], T, dh, rot)
    if scale == "q":
        f32(p + "sc", sv)
        nodes.append(node("Mul", [heads["q"], p + "sc"], [p + "qs"], name=p + "scale_q"))
        heads["q"] = p + "qs"
    elif scale == "sqrt_both":
        f32(p + "sc", math.sqrt(sv))
        nodes += [node("Mul", [heads["q"], p + "sc"], [p + "qs"], name=p + "scale_q"), node("Mul", [heads["k"], p + "sc"], [p + "ks"], name=p + "scale_k")]
        heads["q"], heads["k"] = p + "qs", p + "ks"
    nodes.append(node("MatMul", [heads["q"], heads["k"]], [p + "s0"], name=p + "qk"))
    cur = p + "s0"
    if scale == "scores_div":
        f32(p + "sc", 1.0 / sv)
        nodes.append(node("Div", [cur, p + "sc"], [p + "s1"], name=p + "scale"))
        cur = p + "s1"
    elif scale == "scores_mul":
        f32(p + "sc", sv)
        nodes.append(node("Mul", [cur, p + "sc"], [p + "s1"], name=p + "scale"))
        cur = p + "s1"
    if mask is not None:
        f32(p + "mask", mask)
        nodes.append(node("Add", [p + "mask", cur] if mask_left else [cur, p + "mask"], [p + "s2"], name=p + "mask_add"))
        cur = p + "s2"
    if row_mask is not None:
        cur = row_mask_on_scores(nodes, inits, p, cur, T, h, row_mask, mask_left=mask_left)
    nodes += [node("Softmax", [cur], [p + "p"], [attr_i("axis", softmax_axis)], name=p + "softmax"),
              node("MatMul", [p + "p", heads["v"]], [p + "o4"], name=p + "pv"),
              node("Transpose", [p + "o4"], [p + "ot"], [attr_ints("perm", [0, 2, 1, 3])], name=p + "tr_o"),
              node("Reshape", [p + "ot", p + "merge"], [p + "o"], name=p + "merge_heads")]
    return p + "o"


def row_mask_value(nodes: list, inits: list, p: str, T: int, row_mask: dict) -> str:
    """Appends the part of a row mask's sub-graph that does not depend on the layer and returns its [N, 1, 1, T] value.
    The source row_mask["src"] is an [N, T] graph input: a 0 / 1 mask (HF's attention_mask), or with from_ids = pad_id the token ids.
    form "add" (BERT): kept = src or Not(Equal(ids, pad)) -> Unsqueeze to [N, 1, 1, T] ("one" node, "two" nodes or a "reshape") -> Cast(FLOAT)
        -> Sub(1, .) -> Mul(., fill): the float term added to the scores.
    form "replace" (DistilBERT's masked_fill): masked = Equal(src, 0) or Equal(ids, pad) -> Reshape / Unsqueeze to [N, 1, 1, T]: the condition."""
    form, pad, how = row_mask.get("form", "add"), row_mask.get("from_ids"), row_mask.get("unsqueeze", "one")
    src = row_mask["src"]
    i64 = lambda name, val: inits.append(tensor(name, np.asarray(val, dtype=np.int64)))  # noqa: E731
    i64(p + "rm_c", 0 if pad is None else pad)

    def lift(v):
        if how == "reshape":
            i64(p + "rm_s4", [-1, 1, 1, T])
            nodes.append(node("Reshape", [v, p + "rm_s4"], [p + "rm_4"], name=p + "rm_reshape"))
        elif how == "two":
            i64(p + "rm_a1", [1]); i64(p + "rm_a2", [2])  # noqa: E702
            nodes.extend([node("Unsqueeze", [v, p + "rm_a1"], [p + "rm_3"], name=p + "rm_unsq1"),
                          node("Unsqueeze", [p + "rm_3", p + "rm_a2"], [p + "rm_4"], name=p + "rm_unsq2")])
        else:
            i64(p + "rm_a12", [1, 2])
            nodes.append(node("Unsqueeze", [v, p + "rm_a12"], [p + "rm_4"], name=p + "rm_unsq"))
        return p + "rm_4"

    if form == "replace":
        nodes.append(node("Equal", [src, p + "rm_c"], [p + "rm_eq"], name=p + "rm_equal"))
        return lift(p + "rm_eq")
    kept = src
    if pad is not None:
        nodes += [node("Equal", [src, p + "rm_c"], [p + "rm_eq"], name=p + "rm_equal"), node("Not", [p + "rm_eq"], [p + "rm_keep"], name=p + "rm_not")]
        kept = p + "rm_keep"
    inits.append(tensor(p + "rm_one", np.asarray(1.0, dtype=np.float32)))
    inits.append(tensor(p + "rm_fill", np.asarray(row_mask["fill"], dtype=np.float32)))
    nodes += [node("Cast", [lift(kept)], [p + "rm_f"], [attr_i("to", FLOAT)], name=p + "rm_cast"),
              node("Sub", [p + "rm_one", p + "rm_f"], [p + "rm_inv"], name=p + "rm_sub"),
              node("Mul", [p + "rm_inv", p + "rm_fill"], [p + "rm_term"], name=p + "rm_mul")]
    return p + "rm_term"


def row_mask_on_scores(nodes: list, inits: list, p: str, scores: str, T: int, h: int, row_mask: dict, mask_left: bool = False) -> str:
    """Applies a row mask (row_mask_value; built here unless row_mask["value"] names one built before, the way exporters compute it once for
    every layer) to the scores [N, h, T, T] and returns the masked scores.  "add": Add(scores, term), node '<p>mask_add'; "replace": the
    condition, through an optional Expand to the scores' shape (expand "const": the target [1, h, T, T]; "shape": Shape(scores)), into
    Where(condition, fill, scores), node '<p>mask_where'."""
    val = row_mask.get("value") or row_mask_value(nodes, inits, p, T, row_mask)
    if row_mask.get("form", "add") == "add":
        nodes.append(node("Add", [val, scores] if mask_left else [scores, val], [p + "s3"], name=p + "mask_add"))
        return p + "s3"
    expand = row_mask.get("expand", "none")
    if expand == "const":
        inits.append(tensor(p + "rm_tgt", np.asarray([1, h, T, T], dtype=np.int64)))
        nodes.append(node("Expand", [val, p + "rm_tgt"], [p + "rm_x"], name=p + "rm_expand"))
        val = p + "rm_x"
    elif expand == "shape":
        nodes += [node("Shape", [scores], [p + "rm_tgt"], name=p + "rm_shape"), node("Expand", [val, p + "rm_tgt"], [p + "rm_x"], name=p + "rm_expand")]
        val = p + "rm_x"
    inits.append(tensor(p + "rm_wfill", np.asarray(row_mask["fill"], dtype=np.float32)))
    nodes.append(node("Where", [val, p + "rm_wfill", scores], [p + "s3"], name=p + "mask_where"))
    return p + "s3"


def masked_mean_nodes(nodes: list, inits: list, p: str, x: str, src: str, T: int, E: int, from_ids=None, expand: str = "none", count: str = "m",
                      clip: float = 1e-9) -> str:
    """Appends the masked mean over time of x [N, T, E] (the sentence-embedding head) and returns its [N, E] result, node '<p>div':
    kept = src (a 0 / 1 mask [N, T]) or Not(Equal(ids, from_ids)); m = Cast(FLOAT)(Unsqueeze(kept, -1) [-> Expand to x's shape: "const" target
    [1, T, E] or "shape": Shape(x)]); Mul(x, m) -> ReduceSum(axis 1, keepdims 0); the count: ReduceSum(m, axis 1) (count "m") or
    ReduceSum(Cast(FLOAT)(kept), axis 1, keepdims 1) (count "mask") -> Clip(min = clip); Div."""
    i64 = lambda name, val: inits.append(tensor(name, np.asarray(val, dtype=np.int64)))  # noqa: E731
    kept = src
    if from_ids is not None:
        i64(p + "pad", from_ids)
        nodes += [node("Equal", [src, p + "pad"], [p + "eq"], name=p + "equal"), node("Not", [p + "eq"], [p + "keep"], name=p + "not")]
        kept = p + "keep"
    i64(p + "last", [-1]); i64(p + "t_axis", [1])  # noqa: E702
    nodes.append(node("Unsqueeze", [kept, p + "last"], [p + "k3"], name=p + "unsq"))
    cur = p + "k3"
    if expand == "const":
        i64(p + "tgt", [1, T, E])
        nodes.append(node("Expand", [cur, p + "tgt"], [p + "kx"], name=p + "expand"))
        cur = p + "kx"
    elif expand == "shape":
        nodes += [node("Shape", [x], [p + "tgt"], name=p + "shape"), node("Expand", [cur, p + "tgt"], [p + "kx"], name=p + "expand")]
        cur = p + "kx"
    nodes += [node("Cast", [cur], [p + "m"], [attr_i("to", FLOAT)], name=p + "cast"), node("Mul", [x, p + "m"], [p + "xm"], name=p + "mul"),
              node("ReduceSum", [p + "xm", p + "t_axis"], [p + "sum"], [attr_i("keepdims", 0)], name=p + "sum_x")]
    if count == "m":
        nodes.append(node("ReduceSum", [p + "m", p + "t_axis"], [p + "cnt"], [attr_i("keepdims", 0)], name=p + "sum_m"))
    else:
        nodes += [node("Cast", [kept], [p + "kf"], [attr_i("to", FLOAT)], name=p + "cast_mask"),
                  node("ReduceSum", [p + "kf", p + "t_axis"], [p + "cnt"], [attr_i("keepdims", 1)], name=p + "sum_m")]
    inits.append(tensor(p + "lo", np.asarray(clip, dtype=np.float32)))
    nodes += [node("Clip", [p + "cnt", p + "lo"], [p + "den"], name=p + "clip"), node("Div", [p + "sum", p + "den"], [p + "out"], name=p + "div")]
    return p + "out"


def causal_mask(T: int, rank: int = 2) -> np.ndarray:
    mk = np.triu(np.full((T, T), -np.inf, dtype=np.float32), 1)
    return mk.reshape((1,) * (rank - 2) + (T, T))


def attention_only(T: int, E: int, h: int, form: str = "packed", row_mask: dict | None = None, mask_type: int = INT64, opset: int = 20, **kw) -> bytes:
    """Self-attention alone over a flat input: form "packed": X [N, T*3E] -> Reshape [N, T, 3E] -> Split on the last axis -> q, k, v;
    "three": inputs Q, K, V [N, T*E] each (the call's columns in that order), each reshaped to [N, T, E].  Output [N, T, E].
    row_mask (attention_nodes; its src defaults to "M"): one more input M [N, T] (mask_type: INT64, INT32 or FLOAT) behind the others, the
    0 / 1 mask or, with from_ids, the token ids.  kw: attention_nodes (rotary = ...: with the operator form the model needs opset 23)."""
    nodes, inits = [], []
    if row_mask is not None:
        kw["row_mask"] = dict(row_mask, src=row_mask.get("src", "M"))
    if form == "packed":
        inits += [tensor("x_shape", np.asarray([-1, T, 3 * E], dtype=np.int64)), tensor("sp", np.asarray([E, E, E], dtype=np.int64))]
        nodes += [node("Reshape", ["X", "x_shape"], ["X3"]), node("Split", ["X3", "sp"], ["q", "k", "v"], [attr_i("axis", 2)], name="split_qkv")]
        ins = [value_info("X", ["N", T * 3 * E])]
        xs = "X3"
    else:
        inits.append(tensor("x_shape", np.asarray([-1, T, E], dtype=np.int64)))
        for nm in "qkv":
            nodes.append(node("Reshape", [nm.upper(), "x_shape"], [nm]))
        ins = [value_info(nm, ["N", T * E]) for nm in "QKV"]
        xs = "q"
    if row_mask is not None:
        ins.append(value_info("M", ["N", T], mask_type))
    out = attention_nodes(nodes, inits, "a_", "q", "k", "v", xs, T, E, h, **kw)
    return model("attention", nodes, inits, ins, [value_info(out, ["N", T, E])], opset=opset)


def masked_attention_reference(q, k, v, h: int, keep, fill: float, mode: str = "add", scale: float | None = None, dtype=np.float64) -> np.ndarray:
    """numpy restatement of attention under a per-row key mask keep [N, T] (bool).  float64 (the reference) with the two f32 roundings of the
    operator's definition: the score is fl32(scale . q . k); a masked key's is fl32(that + fill) ("add") or fill ("replace").  float32: the
    same formula evaluated in that format throughout."""
    q, k, v = (np.asarray(a, dtype=dtype) for a in (q, k, v))
    N, T, E = q.shape
    dh = E // h
    sp = lambda a: a.reshape(N, T, h, dh).transpose(0, 2, 1, 3)  # noqa: E731
    keep = np.asarray(keep, dtype=bool).reshape(N, 1, 1, T)
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == np.float64 else (lambda a: a)
    b = dtype(np.float32(fill))
    with np.errstate(all="ignore"):
        s = r32(sp(q) @ sp(k).transpose(0, 1, 3, 2) * dtype((1.0 / math.sqrt(dh)) if scale is None else scale))
        s = np.where(keep, s, r32(s + b) if mode == "add" else np.full_like(s, b))
        s = s - s.max(axis=-1, keepdims=True)
        pr = np.exp(s)
        pr /= pr.sum(axis=-1, keepdims=True)
        return (pr @ sp(v)).transpose(0, 2, 1, 3).reshape(N, T, E)


def masked_mean_reference(x, keep, clip: float = 1e-9) -> np.ndarray:
    """[N, T, E], keep [N, T] -> [N, E] in float64: the sum over the kept steps / max(count, clip)"""
    x, keep = np.asarray(x, dtype=np.float64), np.asarray(keep, dtype=bool)
    return np.where(keep[:, :, None], x, 0.0).sum(axis=1) / np.maximum(keep.sum(axis=1, keepdims=True).astype(np.float64), np.float64(np.float32(clip)))


def attention_reference(q, k, v, h: int, scale: float | None = None, mask=None) -> np.ndarray:
    """float64 numpy restatement of softmax(scale . Q K^T + mask) V per head over q, k, v [N, T, E] -> [N, T, E]."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    N, T, E = q.shape
    dh = E // h
    sp = lambda a: a.reshape(N, T, h, dh).transpose(0, 2, 1, 3)  # noqa: E731
    s = sp(q) @ sp(k).transpose(0, 1, 3, 2) * ((1.0 / math.sqrt(dh)) if scale is None else scale)
    if mask is not None:
        s = s + np.asarray(mask, dtype=np.float64).reshape(T, T)
    s = s - s.max(axis=-1, keepdims=True)
    pr = np.exp(s)
    pr /= pr.sum(axis=-1, keepdims=True)
    return (pr @ sp(v)).transpose(0, 2, 1, 3).reshape(N, T, E)


def layernorm_reference(x, g, b, eps: float) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    d = x - x.mean(axis=-1, keepdims=True)
    y = d / np.sqrt((d * d).mean(axis=-1, keepdims=True) + eps) * np.asarray(g, dtype=np.float64)
    return y if b is None else y + np.asarray(b, dtype=np.float64)


def transformer_reference(spec: dict, x, heads: Sequence[str] = ("mean",)) -> dict:
    """float64 numpy restatement of transformer_from_spec(spec): x [N, T*F] or [N, T, F] -> {output name: array}."""
    from math import erf
    T, F, E, h = spec["T"], spec["F"], spec["E"], spec["h"]
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    x = f64(x).reshape(-1, T, F)
    if spec["Win"] is not None:
        x = x @ f64(spec["Win"]) + f64(spec["bin"])
    if spec["pos"] is not None:
        x = x + f64(spec["pos"]).reshape(1, T, E)
    mask = causal_mask(T) if spec.get("causal") else None
    act = (lambda a: np.maximum(a, 0.0)) if spec["act"] == "Relu" else (lambda a: 0.5 * a * (1.0 + np.vectorize(erf)(a / math.sqrt(2.0))))
    ln = lambda a, g, b: layernorm_reference(a, g, b, spec["eps"])  # noqa: E731
    for L in spec["layers"]:
        a_in = ln(x, L["g1"], L["be1"]) if spec["norm_first"] else x
        a = attention_reference(a_in @ f64(L["Wq"]) + f64(L["bq"]), a_in @ f64(L["Wk"]) + f64(L["bk"]), a_in @ f64(L["Wv"]) + f64(L["bv"]), h, mask=mask)
        x = x + (a @ f64(L["Wo"]) + f64(L["bo"]))
        if not spec["norm_first"]:
            x = ln(x, L["g1"], L["be1"])
        f_in = ln(x, L["g2"], L["be2"]) if spec["norm_first"] else x
        x = x + (act(f_in @ f64(L["W1"]) + f64(L["b1"])) @ f64(L["W2"]) + f64(L["b2"]))
        if not spec["norm_first"]:
            x = ln(x, L["g2"], L["be2"])
    if spec["final_norm"] is not None:
        x = ln(x, spec["final_norm"][0], spec["final_norm"][1])
    out = {}
    for hd in heads:
        v = {"mean": x.mean(axis=1), "first": x[:, 0], "last": x[:, -1], "seq": x}[hd]
        if spec["head_W"] is not None:
            v = v @ f64(spec["head_W"]) + f64(spec["head_b"])
        out["pooled" if hd == "mean" else hd] = v
    return out


def layernorm_nodes(nodes: list, inits: list, x: str, g, b, out: str, name: str, eps: float, form: str = "op") -> str:
    """Appends LayerNorm over the last axis of x: form "op" (LayerNormalization, opset 17) or the decomposed spelling older exporters write,
    ReduceMean(-1) -> Sub -> Pow(2) ("decomposed") or Mul(d, d) ("decomposed_mul") -> ReduceMean(-1) -> Add(eps) -> Sqrt -> Div -> Mul -> Add."""
    f32 = lambda nm, v: inits.append(tensor(nm, np.asarray(v, dtype=np.float32)))  # noqa: E731
    f32(name + "_g", g)
    if b is not None:
        f32(name + "_b", b)
    if form == "op":
        nodes.append(node("LayerNormalization", [x, name + "_g"] + ([name + "_b"] if b is not None else []), [out], [attr_i("axis", -1), attr_f("epsilon", eps)], name=name))
        return out
    inits.append(tensor(name + "_ax", np.asarray([-1], dtype=np.int64)))
    f32(name + "_eps", eps)
    p = name + "_"
    nodes += [node("ReduceMean", [x, name + "_ax"], [p + "mu"], [attr_i("keepdims", 1)], name=p + "mean"), node("Sub", [x, p + "mu"], [p + "d"], name=p + "sub")]
    if form == "decomposed":
        f32(name + "_two", 2.0)
        nodes.append(node("Pow", [p + "d", name + "_two"], [p + "sq"], name=p + "pow"))
    else:
        nodes.append(node("Mul", [p + "d", p + "d"], [p + "sq"], name=p + "square"))
    nodes += [node("ReduceMean", [p + "sq", name + "_ax"], [p + "var"], [attr_i("keepdims", 1)], name=p + "var"),
              node("Add", [p + "var", name + "_eps"], [p + "ve"], name=p + "eps"), node("Sqrt", [p + "ve"], [p + "sd"], name=p + "sqrt"),
              node("Div", [p + "d", p + "sd"], [p + "nrm"], name=p + "div"), node("Mul", [p + "nrm", name + "_g"], [p + "sc"] if b is not None else [out], name=p + "gamma")]
    if b is not None:
        nodes.append(node("Add", [p + "sc", name + "_b"], [out], name=p + "beta"))
    return out


def transformer_from_spec(spec: dict, flat: bool = True, qkv: str = "separate", scale: str = "scores_div", k_transpose: str = "direct",
                          mask_rank: int = 2, shape: str = "const", gelu: str = "op", heads: Sequence[str] = ("mean",), keepdims: int = 0,
                          opset: int = 20, layernorm: str = "op", pos_rank: int = 3, front: tuple | None = None, row_mask: dict | None = None,
                          mean_mask: dict | None = None) -> bytes:
    """The ONNX model of a transformer_spec() / from_torch_encoder() dict, input X [N, T, F] (flat: [N, T*F] -> Reshape).
    qkv: "separate" (three MatMul + Add), "packed_split" / "packed_slice" (one [E, 3E] projection, then Split / three Slices on the last axis);
    scale, k_transpose, shape: see attention_nodes; a causal spec adds the [T, T] mask (mask_rank 4: [1, 1, T, T]); gelu: "op" (opset 20) or
    "decomposed" (Div(sqrt 2) -> Erf -> Add(1) -> Mul(x) -> Mul(0.5)).  heads: the graph outputs, any of "mean" (mean over time -> Linear,
    output "pooled"), "first" / "last" (that step -> Linear), "seq" (the full sequence [N, T, E] -> per-step Linear); without a head matrix
    in the spec the encoder output itself is served.  layernorm: see layernorm_nodes ("op" is the default); pos_rank: the positional constant as [1, T, E] or [T, E].
    front: (nodes, initializers, name of the [N, T, E] value they compute, graph inputs) -- the encoder then starts from that value (vit_from_spec).
    row_mask: every layer's attention under that per-row key mask (attention_nodes); its layer-independent part is computed once, the way
    exporters write it.  mean_mask: the keyword arguments of masked_mean_nodes behind x, for the head "masked_mean" (output "sentence")."""
    T, F, E, h, ff = spec["T"], spec["F"], spec["E"], spec["h"], spec["ff"]
    nodes, inits = (list(front[0]), list(front[1])) if front else ([], [])
    i64 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.int64)))  # noqa: E731
    f32 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.float32)))  # noqa: E731

    def linear(x, W, b, out, name):
        f32(name + "_W", W)
        f32(name + "_b", b)
        nodes.append(node("MatMul", [x, name + "_W"], [out + "_mm"], name=name))
        nodes.append(node("Add", [out + "_mm", name + "_b"], [out], name=name + "_bias"))
        return out

    def layer_norm(x, g, b, out, name):
        return layernorm_nodes(nodes, inits, x, g, b, out, name, spec["eps"], layernorm)

    x = front[2] if front else "X"
    if flat and not front:
        i64("flat_shape", [-1, T, F])
        nodes.append(node("Reshape", [x, "flat_shape"], ["X3"]))
        x = "X3"
    if spec["Win"] is not None:
        x = linear(x, spec["Win"], spec["bin"], "emb", "in_proj")
    if spec["pos"] is not None:
        f32("pos", np.asarray(spec["pos"]).reshape((1, T, E) if pos_rank == 3 else (T, E)))
        nodes.append(node("Add", [x, "pos"], ["emb_pos"], name="pos_add"))
        x = "emb_pos"
    mask = causal_mask(T, mask_rank) if spec.get("causal") else None
    attn_kw = {}
    if row_mask is not None:
        attn_kw["row_mask"] = dict(row_mask, value=row_mask_value(nodes, inits, "rm_", T, row_mask))
    for i, L in enumerate(spec["layers"]):
        p = f"l{i}_"
        a_in = layer_norm(x, L["g1"], L["be1"], p + "n1", p + "norm1") if spec["norm_first"] else x
        if qkv == "separate":
            q, k, v = (linear(a_in, L["W" + c], L["b" + c], p + c, p + c + "_proj") for c in "qkv")
        else:
            linear(a_in, np.concatenate([L["Wq"], L["Wk"], L["Wv"]], axis=1), np.concatenate([L["bq"], L["bk"], L["bv"]]), p + "qkv", p + "qkv_proj")
            q, k, v = p + "q", p + "k", p + "v"
            if qkv == "packed_split":
                i64(p + "sp", [E, E, E])
                nodes.append(node("Split", [p + "qkv", p + "sp"], [q, k, v], [attr_i("axis", -1)], name=p + "split_qkv"))
            else:
                i64(p + "ax2", [2])
                for j, nm in enumerate((q, k, v)):
                    i64(nm + "_b", [j * E]); i64(nm + "_e", [(j + 1) * E])  # noqa: E702
                    nodes.append(node("Slice", [p + "qkv", nm + "_b", nm + "_e", p + "ax2"], [nm], name=nm + "_slice"))
        a = attention_nodes(nodes, inits, p + "a_", q, k, v, a_in, T, E, h, scale=scale, k_transpose=k_transpose, mask=mask, shape=shape, **attn_kw)
        a = linear(a, L["Wo"], L["bo"], p + "ao", p + "out_proj")
        nodes.append(node("Add", [x, a], [p + "r1"], name=p + "res1"))
        x = p + "r1"
        if not spec["norm_first"]:
            x = layer_norm(x, L["g1"], L["be1"], p + "n1", p + "norm1")
        f_in = layer_norm(x, L["g2"], L["be2"], p + "n2", p + "norm2") if spec["norm_first"] else x
        hdn = linear(f_in, L["W1"], L["b1"], p + "f1", p + "ff1")
        if spec["act"] == "Gelu" and gelu == "decomposed":
            f32(p + "sqrt2", math.sqrt(2.0)); f32(p + "one", 1.0); f32(p + "half", 0.5)  # noqa: E702
            nodes += [node("Div", [hdn, p + "sqrt2"], [p + "g0"]), node("Erf", [p + "g0"], [p + "g1"]), node("Add", [p + "g1", p + "one"], [p + "g2"]),
                      node("Mul", [hdn, p + "g2"], [p + "g3"]), node("Mul", [p + "g3", p + "half"], [p + "fa"])]
        else:
            nodes.append(node(spec["act"], [hdn], [p + "fa"], name=p + "act"))
        f = linear(p + "fa", L["W2"], L["b2"], p + "f2", p + "ff2")
        nodes.append(node("Add", [x, f], [p + "r2"], name=p + "res2"))
        x = p + "r2"
        if not spec["norm_first"]:
            x = layer_norm(x, L["g2"], L["be2"], p + "n2", p + "norm2")
    if spec["final_norm"] is not None:
        x = layer_norm(x, spec["final_norm"][0], spec["final_norm"][1], "enc", "final_norm")
    M = None if spec["head_W"] is None else int(np.asarray(spec["head_W"]).shape[1])
    outs = []
    for hd in heads:
        if hd == "mean":
            i64("t_axis", [1])
            nodes.append(node("ReduceMean", [x, "t_axis"], ["mean_t"], [attr_i("keepdims", keepdims)], name="mean_over_time"))
            v, dims, name = "mean_t", (["N", 1, E] if keepdims else ["N", E]), "pooled"
        elif hd == "masked_mean":
            v, dims, name = masked_mean_nodes(nodes, inits, "mm_", x, T=T, E=E, **mean_mask), ["N", E], "sentence"
        elif hd in ("first", "last"):
            i64(hd + "_i", 0 if hd == "first" else -1)
            nodes.append(node("Gather", [x, hd + "_i"], [hd + "_t"], [attr_i("axis", 1)], name=hd + "_step"))
            v, dims, name = hd + "_t", ["N", E], hd
        else:
            v, dims, name = x, ["N", T, E], "seq"
        if M is not None:
            linear(v, spec["head_W"], spec["head_b"], name, name + "_head")
            dims = dims[:-1] + [M]
        else:
            nodes.append(node("Identity", [v], [name]))
        outs.append(value_info(name, dims))
    in_dims = ["N", T * F] if flat else ["N", T, F]
    return model("transformer", nodes, inits, list(front[3]) if front else [value_info("X", in_dims)], outs, opset=opset)


# ------------------------------------------------------------------------------------------
# ai.onnx.ml preprocessing (Imputer, Scaler, OneHotEncoder, LabelEncoder, Binarizer, ArrayFeatureExtractor, Concat, ZipMap)
# ------------------------------------------------------------------------------------------

def value_info_zipmap(name: str, key_type: int = INT64) -> bytes:
    """A ZipMap output: sequence(map(key_type, float))."""
    tensor_f = _ld(1, _vi(1, FLOAT))
    map_t = _ld(5, _vi(1, key_type) + _ld(2, tensor_f))
    return _s(1, name) + _ld(2, _ld(4, _ld(1, map_t)))


def prep_spec(numeric: int = 6, categorical: int = 8, cats_total: int = 100, ordinal: int = 2, ordinal_keys: int = 20,
              binarized: int = 0, strict: bool = False, seed: int = 11) -> dict:
    """Seeded ColumnTransformer-like preprocessing: `numeric` columns through Imputer (NaN -> a value) and Scaler, `categorical` columns
    one-hot encoded with `cats_total` integer categories in all (some negative), `ordinal` columns through a LabelEncoder of
    `ordinal_keys` integer keys each (alternately keys_int64s and keys_floats), `binarized` columns through a Binarizer.  The columns of
    each group are scattered over the input (non-contiguous ArrayFeatureExtractor indices).  strict: OneHotEncoder zeros = 0."""
    rng = np.random.default_rng(seed)
    F_in = numeric + categorical + ordinal + binarized
    perm = [int(v) for v in rng.permutation(F_in)]
    groups, at = {}, 0
    for g, n in (("numeric", numeric), ("categorical", categorical), ("ordinal", ordinal), ("binarized", binarized)):
        groups[g] = perm[at:at + n]
        at += n
    per = np.full(categorical, cats_total // max(categorical, 1))
    per[:cats_total - int(per.sum())] += 1
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    cats = [sorted(int(v) for v in rng.choice(np.arange(-20, 40), int(c), replace=False)) for c in per]
    ordinal_tabs = []
    for i in range(ordinal):
        keys = sorted(int(v) for v in rng.choice(np.arange(-10, 50), ordinal_keys, replace=False))
        ordinal_tabs.append({"keys": keys, "values": f32(rng.permutation(ordinal_keys)), "default": -1.0, "floats": i % 2 == 1})
    return {
        "features": F_in, "groups": groups, "strict": strict,
        "imputed": f32(rng.normal(0, 1, numeric)), "offset": f32(rng.normal(0, 1, numeric)), "scale": f32(rng.uniform(0.5, 2, numeric)),
        "cats": cats, "ordinal": ordinal_tabs, "thresholds": f32(rng.normal(0, 0.5, binarized)),
    }


def prep_width(spec: dict) -> int:
    """F': the columns prep_from_spec's Concat produces."""
    return len(spec["groups"]["numeric"]) + sum(len(c) for c in spec["cats"]) + len(spec["ordinal"]) + len(spec["groups"]["binarized"])


def prep_nodes(spec: dict, x: str = "X", out: str = "features", after_onehot: str = "Reshape", cast: bool = True,
               concat_axis: int = 1) -> tuple[list, list]:
    """The preprocessing nodes of a prep_spec() dict, laid out as skl2onnx writes a ColumnTransformer: one ArrayFeatureExtractor per
    column group (numeric) or column (categorical / ordinal), Imputer -> Scaler, [Cast(int64) ->] OneHotEncoder -> Reshape([-1, C])
    (or Flatten / Squeeze(axis 1)), LabelEncoder, Binarizer, then Concat.  Returns (nodes, initializers)."""
    nodes, inits, parts = [], [], []
    g = spec["groups"]

    def afe(cols, name):
        inits.append(tensor(name + "_idx", np.asarray(cols, dtype=np.int64)))
        nodes.append(node("ArrayFeatureExtractor", [x, name + "_idx"], [name + "_cols"], name=name + "_afe", domain=ML_DOMAIN))
        return name + "_cols"

    if g["numeric"]:
        v = afe(g["numeric"], "num")
        nodes.append(node("Imputer", [v], ["num_imp"], [attr_floats("imputed_value_floats", spec["imputed"]),
                                                        attr_f("replaced_value_float", float("nan"))], name="num_imputer", domain=ML_DOMAIN))
        nodes.append(node("Scaler", ["num_imp"], ["num_scaled"], [attr_floats("offset", spec["offset"]), attr_floats("scale", spec["scale"])],
                          name="num_scaler", domain=ML_DOMAIN))
        parts.append("num_scaled")
    for i, (col, cats) in enumerate(zip(g["categorical"], spec["cats"])):
        v = afe([col], f"cat{i}")
        if cast:
            nodes.append(node("Cast", [v], [f"cat{i}_int"], [attr_i("to", INT64)], name=f"cat{i}_cast"))
            v = f"cat{i}_int"
        nodes.append(node("OneHotEncoder", [v], [f"cat{i}_oh"], [attr_ints("cats_int64s", cats), attr_i("zeros", 0 if spec["strict"] else 1)],
                          name=f"cat{i}_onehot", domain=ML_DOMAIN))
        if after_onehot == "Reshape":
            inits.append(tensor(f"cat{i}_shape", np.asarray([-1, len(cats)], dtype=np.int64)))
            nodes.append(node("Reshape", [f"cat{i}_oh", f"cat{i}_shape"], [f"cat{i}_flat"], name=f"cat{i}_reshape"))
        elif after_onehot == "Flatten":
            nodes.append(node("Flatten", [f"cat{i}_oh"], [f"cat{i}_flat"], [attr_i("axis", 1)], name=f"cat{i}_flatten"))
        else:
            inits.append(tensor(f"cat{i}_axes", np.asarray([1], dtype=np.int64)))
            nodes.append(node("Squeeze", [f"cat{i}_oh", f"cat{i}_axes"], [f"cat{i}_flat"], name=f"cat{i}_squeeze"))
        parts.append(f"cat{i}_flat")
    for i, (col, t) in enumerate(zip(g["ordinal"], spec["ordinal"])):
        v = afe([col], f"ord{i}")
        keys = attr_floats("keys_floats", t["keys"]) if t["floats"] else attr_ints("keys_int64s", t["keys"])
        nodes.append(node("LabelEncoder", [v], [f"ord{i}_enc"], [keys, attr_floats("values_floats", t["values"]),
                                                                 attr_f("default_float", t["default"])], name=f"ord{i}_encoder", domain=ML_DOMAIN))
        parts.append(f"ord{i}_enc")
    for i, (col, thr) in enumerate(zip(g["binarized"], spec["thresholds"])):
        v = afe([col], f"bin{i}")
        nodes.append(node("Binarizer", [v], [f"bin{i}_b"], [attr_f("threshold", float(thr))], name=f"bin{i}_binarizer", domain=ML_DOMAIN))
        parts.append(f"bin{i}_b")
    nodes.append(node("Concat", parts, [out], [attr_i("axis", concat_axis)], name="concat"))
    return nodes, inits


def prep_from_spec(spec: dict, head=None, zipmap: bool = False, **layout) -> bytes:
    """The ONNX model of a prep_spec() dict: the preprocessing nodes (prep_nodes, `layout` keywords) and, when given, an estimator `head`
    reading their output (a callable (x, F') -> (nodes, initializers, outputs): tree_head / svm_head / linear_head).  Without a head the
    graph serves the preprocessed rows [N, F'].  zipmap: a ZipMap on the head's probabilities, output 'output_probability'."""
    nodes, inits = prep_nodes(spec, **layout)
    Fp = prep_width(spec)
    if head is None:
        outs = [value_info("features", ["N", Fp])]
    else:
        hn, hi, outs = head("features", Fp)
        nodes, inits = nodes + hn, inits + hi
    if zipmap:
        nodes.append(node("ZipMap", ["probabilities"], ["output_probability"], [attr_ints("classlabels_int64s", head.labels)], name="zipmap",
                          domain=ML_DOMAIN))
        outs = [outs[0], value_info_zipmap("output_probability")]
    return model("prep", nodes, inits, [value_info("X", ["N", spec["features"]])], outs, opset=13, ml_opset=3)


class _Head:
    """An estimator graph reading the preprocessed rows: call (x, F) -> (nodes, initializers, outputs [label, probabilities] or [Y])."""

    def __init__(self, build, labels=None):
        self.build, self.labels = build, labels

    def __call__(self, x: str, F: int):
        return self.build(x, F)


def tree_head(spec: dict) -> _Head:
    """A tree_ensemble_spec()-style dict (its "features" = F') as a head."""
    def build(x, F):
        assert spec["features"] == F, (spec["features"], F)
        nd, (a, b) = _tree_node(spec, x)
        return [nd], [], [a, b] if b is not None else [a]
    return _Head(build, list(spec.get("labels", [])))


def svm_head(spec: dict) -> _Head:
    """An svm_spec()-style dict (its "features" = F') as a head."""
    def build(x, F):
        assert spec["features"] == F, (spec["features"], F)
        nd, (a, b) = _svm_node(spec, x)
        return [nd], [], [a, b] if b is not None else [a]
    return _Head(build, list(spec.get("labels", [])))


def linear_head(coef, intercepts, labels: Sequence[int], post: str = "SOFTMAX") -> _Head:
    """LinearClassifier(coefficients [C, F'], intercepts [C]) as a head."""
    coef = np.asarray(coef, dtype=np.float32)

    def build(x, F):
        assert coef.shape[1] == F, (coef.shape, F)
        nd = node("LinearClassifier", [x], ["label", "probabilities"],
                  [attr_floats("coefficients", coef.ravel()), attr_floats("intercepts", np.asarray(intercepts, np.float32)),
                   attr_ints("classlabels_ints", labels), attr_s("post_transform", post)], domain=ML_DOMAIN)
        return [nd], [], [value_info("label", ["N"], INT64), value_info("probabilities", ["N", len(labels)])]
    return _Head(build, list(labels))


def sklearn_tree_spec(est, F: int) -> dict:
    """A fitted RandomForestClassifier / RandomForestRegressor / GradientBoostingRegressor as a tree_ensemble_spec()-style dict."""
    cls = hasattr(est, "classes_")
    gb = hasattr(est, "init_")
    trees = [e[0].tree_ for e in est.estimators_] if gb else [e.tree_ for e in est.estimators_]
    E = len(est.classes_) if cls else 1
    scale = float(est.learning_rate) if gb else 1.0
    keys = ("nodes_treeids", "nodes_nodeids", "nodes_featureids", "nodes_modes", "nodes_values", "nodes_truenodeids", "nodes_falsenodeids")
    nd = {k: [] for k in keys}
    lt, ln, lid, lw = [], [], [], []
    for t, tr in enumerate(trees):
        for i in range(tr.node_count):
            leaf = tr.children_left[i] < 0
            for k, v in zip(keys, (t, i, 0 if leaf else int(tr.feature[i]), "LEAF" if leaf else "BRANCH_LEQ",
                                   0.0 if leaf else float(tr.threshold[i]), 0 if leaf else int(tr.children_left[i]),
                                   0 if leaf else int(tr.children_right[i]))):
                nd[k].append(v)
            if leaf:
                v = tr.value[i].ravel()
                if cls:
                    v = v / v.sum()
                for j in range(E):
                    lt.append(t), ln.append(i), lid.append(j), lw.append(float(v[j]) * scale)
    spec = {"kind": "classifier" if cls else "regressor", "features": F, "E": E,
            "labels": [int(c) for c in est.classes_] if cls else [0], "aggregate": "SUM" if gb else "AVERAGE", "post": "NONE",
            "as_tensor": True, "missing": False, "leaf_treeids": lt, "leaf_nodeids": ln, "leaf_ids": lid, "leaf_weights": np.array(lw),
            "base_values": np.array([float(est.init_.constant_.ravel()[0])]) if gb else None}
    spec.update(nd)
    spec["nodes_values"] = np.array(spec["nodes_values"])
    return spec


def sklearn_svm_spec(est, F: int) -> dict:
    """A fitted SVC as an svm_spec()-style dict (libsvm's one-vs-one layout)."""
    spec = {"kind": "classifier", "features": F, "kernel": est.kernel.upper(), "post": "NONE", "n_sv": int(est.support_vectors_.shape[0]),
            "support_vectors": np.asarray(est.support_vectors_, dtype=np.float32),
            "coefficients": np.asarray(est._dual_coef_, dtype=np.float32), "rho": np.asarray(est._intercept_, dtype=np.float32).ravel(),
            "kernel_params": np.asarray([est._gamma, est.coef0, est.degree], dtype=np.float32), "prob_a": None, "prob_b": None,
            "classes": len(est.classes_), "labels": [int(c) for c in est.classes_], "vectors_per_class": [int(v) for v in est.n_support_]}
    return spec


def sklearn_column_transformer(ct, estimator_graph=None, zipmap: bool = False, after_onehot: str = "Reshape", cast: bool = True,
                               concat_axis: int = 1) -> bytes:
    """A fitted sklearn ColumnTransformer [+ estimator] as ONNX, laid out the way skl2onnx writes it (from the operator specifications
    and the converter's known layout, not from skl2onnx itself): per transformer an ArrayFeatureExtractor of its columns, then
    Pipeline(SimpleImputer, StandardScaler) -> Imputer -> Scaler; OneHotEncoder -> per column [Cast(int64) ->] OneHotEncoder ->
    Reshape([-1, C]); OrdinalEncoder -> per column LabelEncoder; Binarizer; 'passthrough'; all joined by Concat.  The input is one f32
    matrix X [N, n_features_in_].  estimator_graph: a head (tree_head / svm_head / linear_head) over the F' transformed columns, else
    the transformed rows are the output.  zipmap: a ZipMap on the head's probabilities."""
    nodes, inits, parts, Fp = [], [], [], 0
    uid = [0]

    def fresh(p):
        uid[0] += 1
        return f"{p}{uid[0]}"

    def afe(cols):
        n = fresh("afe")
        inits.append(tensor(n + "_idx", np.asarray(cols, dtype=np.int64)))
        nodes.append(node("ArrayFeatureExtractor", ["X", n + "_idx"], [n], name=n, domain=ML_DOMAIN))
        return n

    def cols_of(sel):
        idx = np.arange(ct.n_features_in_)[sel] if not isinstance(sel, (list, tuple)) or isinstance(sel, slice) else np.asarray(sel)
        return [int(c) for c in np.atleast_1d(idx)]

    for name, tr, sel in ct.transformers_:
        if tr == "drop":
            continue
        cols = cols_of(sel)
        if not cols:
            continue
        steps = [s for _, s in tr.steps] if hasattr(tr, "steps") else [tr]
        kinds = [type(s).__name__ for s in steps]
        if tr == "passthrough":
            parts.append(afe(cols))
            Fp += len(cols)
        elif set(kinds) <= {"SimpleImputer", "StandardScaler"}:
            v = afe(cols)
            for s in steps:
                o = fresh(type(s).__name__)
                if type(s).__name__ == "SimpleImputer":
                    nodes.append(node("Imputer", [v], [o], [attr_floats("imputed_value_floats", np.asarray(s.statistics_, np.float32)),
                                                            attr_f("replaced_value_float", float("nan"))], name=o, domain=ML_DOMAIN))
                else:
                    mean = s.mean_ if s.with_mean else np.zeros(len(cols))
                    sc = 1.0 / s.scale_ if s.with_std else np.ones(len(cols))
                    nodes.append(node("Scaler", [v], [o], [attr_floats("offset", np.asarray(mean, np.float32)),
                                                          attr_floats("scale", np.asarray(sc, np.float32))], name=o, domain=ML_DOMAIN))
                v = o
            parts.append(v)
            Fp += len(cols)
        elif kinds == ["OneHotEncoder"]:
            enc = steps[0]
            if getattr(enc, "drop_idx_", None) is not None or getattr(enc, "infrequent_categories_", None) is not None:
                raise TypeError(f"transformer {name!r}: OneHotEncoder with drop= or infrequent categories is not written by this builder")
            for j, c in enumerate(cols):
                v = afe([c])
                if cast:
                    o = fresh("cast")
                    nodes.append(node("Cast", [v], [o], [attr_i("to", INT64)], name=o))
                    v = o
                cats = [int(k) for k in enc.categories_[j]]
                o = fresh("onehot")
                nodes.append(node("OneHotEncoder", [v], [o], [attr_ints("cats_int64s", cats),
                                                             attr_i("zeros", 0 if enc.handle_unknown == "error" else 1)], name=o, domain=ML_DOMAIN))
                f = fresh("flat")
                if after_onehot == "Reshape":
                    inits.append(tensor(f + "_shape", np.asarray([-1, len(cats)], dtype=np.int64)))
                    nodes.append(node("Reshape", [o, f + "_shape"], [f], name=f))
                elif after_onehot == "Flatten":
                    nodes.append(node("Flatten", [o], [f], [attr_i("axis", 1)], name=f))
                else:
                    inits.append(tensor(f + "_axes", np.asarray([1], dtype=np.int64)))
                    nodes.append(node("Squeeze", [o, f + "_axes"], [f], name=f))
                parts.append(f)
                Fp += len(cats)
        elif kinds == ["OrdinalEncoder"]:
            enc = steps[0]
            unknown = getattr(enc, "unknown_value", None)
            for j, c in enumerate(cols):
                v = afe([c])
                cats = [int(k) for k in enc.categories_[j]]
                o = fresh("ordinal")
                nodes.append(node("LabelEncoder", [v], [o], [attr_ints("keys_int64s", cats),
                                                            attr_floats("values_floats", np.arange(len(cats), dtype=np.float32)),
                                                            attr_f("default_float", float(unknown) if unknown is not None else -1.0)],
                                  name=o, domain=ML_DOMAIN))
                parts.append(o)
                Fp += 1
        elif kinds == ["Binarizer"]:
            v = afe(cols)
            o = fresh("binarizer")
            nodes.append(node("Binarizer", [v], [o], [attr_f("threshold", float(steps[0].threshold))], name=o, domain=ML_DOMAIN))
            parts.append(o)
            Fp += len(cols)
        else:
            raise TypeError(f"transformer {name!r}: {kinds} is not written by this builder")
    nodes.append(node("Concat", parts, ["features"], [attr_i("axis", concat_axis)], name="concat"))
    if estimator_graph is None:
        outs = [value_info("features", ["N", Fp])]
    else:
        hn, hi, outs = estimator_graph("features", Fp)
        nodes, inits = nodes + hn, inits + hi
    if zipmap:
        nodes.append(node("ZipMap", ["probabilities"], ["output_probability"], [attr_ints("classlabels_int64s", estimator_graph.labels)],
                          name="zipmap", domain=ML_DOMAIN))
        outs = [outs[0], value_info_zipmap("output_probability")]
    return model("column_transformer", nodes, inits, [value_info("X", ["N", int(ct.n_features_in_)])], outs, opset=13, ml_opset=3)


# ------------------------------------------------------------------------------------------
# statically quantised MLPs (QDQ and QLinearMatMul spellings) and their numpy references
# ------------------------------------------------------------------------------------------

def _qrange(t: str) -> tuple[int, int]:
    return (-128, 127) if t == "int8" else (0, 255)


def _calibrate(lo: float, hi: float, t: str) -> tuple[np.float32, int]:
    """Asymmetric per-tensor parameters whose range covers [min(lo, 0), max(hi, 0)]."""
    qmin, qmax = _qrange(t)
    lo, hi = min(float(lo), 0.0), max(float(hi), 0.0)
    scale = np.float32(max(hi - lo, 1e-6) / (qmax - qmin))
    zp = int(np.clip(np.rint(qmin - lo / float(scale)), qmin, qmax))
    return scale, zp


def _float_act(h, act):
    if act == "Relu":
        return np.maximum(h, 0)
    if isinstance(act, tuple):  # ("Clip", lo, hi)
        return np.clip(h, act[1], act[2])
    return h


def quantized_mlp_spec(dims: Sequence[int] = (128, 256, 64, 1), acts: Sequence | None = None, x_type: str = "uint8", w_type: str = "int8",
                       per_channel: bool = True, w_zero_points: bool = False, bias: str | None = "int32", seed: int = 1234,
                       x_zero_point: int | None = None, tail: str = "", calib_rows: int = 256) -> dict:
    """A Gemm chain with the weights of mlp() quantised the way ONNX Runtime's quantize_static does: weights per tensor or per output
    channel (symmetric, or with zero points where w_zero_points), activations per tensor, their ranges taken from the float network
    on `calib_rows` rows of the synthetic table.  acts[l]: "" | "Relu" | ("Clip", lo, hi).  bias: "int32" (scale x_scale * w_scale,
    zero point 0), "f32" or None.  spec["q"][l] = (scale, zero point) of the input of layer l; [-1]: of the network's result."""
    nl = len(dims) - 1
    acts = list(acts) if acts is not None else ["Relu"] * (nl - 1) + [""]
    assert len(acts) == nl and w_type in ("int8", "uint8") and x_type in ("int8", "uint8") and bias in ("int32", "f32", None)
    from .synth import table
    ws = _WeightStream(seed)
    h = table(seed + 1, 0, calib_rows, dims[0]).astype(np.float64)
    q = [_calibrate(h.min(), h.max(), x_type)]
    if x_zero_point is not None:
        q[0] = (q[0][0], int(x_zero_point))
    wmin, wmax = _qrange(w_type)
    layers = []
    for l in range(nl):
        k, m = dims[l], dims[l + 1]
        w = ws.take((k, m), k).astype(np.float64)
        b = ws.take((m,), k).astype(np.float64)
        cols = w if per_channel else w.reshape(-1, 1)
        if w_zero_points:
            lo, hi = np.minimum(cols.min(0), 0), np.maximum(cols.max(0), 0)
            w_scale = (np.maximum(hi - lo, 1e-6) / (wmax - wmin)).astype(np.float32)
            w_zp = np.clip(np.rint(wmin - lo / w_scale), wmin, wmax).astype(np.int64)
        else:
            w_scale = (np.maximum(np.abs(cols).max(0), 1e-6) / 127.0).astype(np.float32)
            w_zp = np.full(w_scale.shape, 0 if w_type == "int8" else 128, np.int64)
        wq = np.clip(np.rint(w / w_scale.astype(np.float64)) + w_zp, wmin, wmax).astype(np.int64)
        layer = {"wq": wq, "w_scale": w_scale, "w_zp": w_zp, "bias_q": None, "bias_f": None}
        if bias == "int32":
            layer["bias_scale"] = (q[l][0] * w_scale).astype(np.float32)  # the f32 product, as the loader forms it
            layer["bias_q"] = np.rint(b / np.broadcast_to(layer["bias_scale"].astype(np.float64), (m,))).astype(np.int64)
        elif bias == "f32":
            layer["bias_f"] = b.astype(np.float32)
        layers.append(layer)
        h = _float_act(h @ ((wq - w_zp) * w_scale.astype(np.float64)) + (b if bias else 0.0), acts[l])
        q.append(_calibrate(h.min(), h.max(), x_type))
    return {"dims": list(dims), "acts": acts, "x_type": x_type, "w_type": w_type, "per_channel": per_channel, "layers": layers, "q": q, "tail": tail}


def _np_qtype(t: str):
    return np.int8 if t == "int8" else np.uint8


def quantized_from_spec(spec: dict, form: str = "qdq", layer: str = "matmul_add", weight_only: bool = False, int32_data: bool = False,
                        batch: int | str = "N", window: int = 0) -> bytes:
    """The network of a quantized_mlp_spec as a QDQ graph (QuantizeLinear / DequantizeLinear around float MatMul + Add or Gemm; layer =
    "matmul_add" | "gemm" | "gemm_transb") or in the QOperator spelling (form="qlinear": QuantizeLinear -> QLinearMatMul ... ->
    DequantizeLinear; no bias, and only activations that the next quantisation's range already applies).  weight_only: only the
    weights are quantised.  window = T > 0: the input [N, T * dims[0]] is reshaped to [N, T, dims[0]] and every layer runs on each of its T vectors (MatMul forms)."""
    dims, acts, layers, q = spec["dims"], spec["acts"], spec["layers"], spec["q"]
    xt, wt = _np_qtype(spec["x_type"]), _np_qtype(spec["w_type"])
    qmin = _qrange(spec["x_type"])[0]
    nodes, inits = [], []

    def scalar(name, v, dtype):
        inits.append(tensor(name, np.array(v, dtype), int32_data=int32_data and dtype != np.float32))
        return name

    def wparams(l):
        L = layers[l]
        pc = spec["per_channel"]
        inits.append(tensor(f"W{l}_scale", L["w_scale"].astype(np.float32) if pc else np.array(L["w_scale"][0], np.float32)))
        inits.append(tensor(f"W{l}_zp", L["w_zp"].astype(wt) if pc else np.array(L["w_zp"][0], wt), int32_data=int32_data))
        return f"W{l}_scale", f"W{l}_zp"

    cur = "X"
    if window:
        inits.append(tensor("window_shape", np.array([-1, window, dims[0]], np.int64)))
        nodes.append(node("Reshape", ["X", "window_shape"], ["X3"], name="window"))
        cur = "X3"
    if form == "qlinear":
        assert not weight_only
        nodes.append(node("QuantizeLinear", [cur, scalar("q0_scale", q[0][0], np.float32), scalar("q0_zp", q[0][1], xt)], ["Xq"], name="quant_in"))
        cur = "Xq"
        for l, L in enumerate(layers):
            if L["bias_q"] is not None or L["bias_f"] is not None:
                raise ValueError("QLinearMatMul carries no bias")
            if acts[l] and not (acts[l] == "Relu" and q[l + 1][1] == qmin):
                raise ValueError("the QLinear spelling cannot express activation %r before zero point %d" % (acts[l], q[l + 1][1]))
            inits.append(tensor(f"W{l}", L["wq"].astype(wt), int32_data=int32_data))
            wsn, wzn = wparams(l)
            nodes.append(node("QLinearMatMul", [cur, f"q{l}_scale", f"q{l}_zp", f"W{l}", wsn, wzn, scalar(f"q{l + 1}_scale", q[l + 1][0], np.float32),
                                                scalar(f"q{l + 1}_zp", q[l + 1][1], xt)], [f"H{l}q"], name=f"qmm{l}"))
            cur = f"H{l}q"
        out = "Yf" if spec["tail"] else "Y"
        nodes.append(node("DequantizeLinear", [cur, f"q{len(layers)}_scale", f"q{len(layers)}_zp"], [out], name="dequant_out"))
        cur = out
    else:
        def fake_quant(x, i, out):
            sn, zn = scalar(f"q{i}_scale", q[i][0], np.float32), scalar(f"q{i}_zp", q[i][1], xt)
            nodes.append(node("QuantizeLinear", [x, sn, zn], [f"{out}_q"], name=f"quant{i}"))
            nodes.append(node("DequantizeLinear", [f"{out}_q", sn, zn], [out], name=f"dequant{i}"))
            return out
        if not weight_only:
            cur = fake_quant(cur, 0, "X_dq")
        for l, L in enumerate(layers):
            k, m = dims[l], dims[l + 1]
            trans = layer == "gemm_transb"
            inits.append(tensor(f"W{l}", np.ascontiguousarray(L["wq"].T if trans else L["wq"]).astype(wt), int32_data=int32_data))
            wsn, wzn = wparams(l)
            axis = 0 if trans else 1
            nodes.append(node("DequantizeLinear", [f"W{l}", wsn, wzn], [f"W{l}_dq"], [attr_i("axis", axis)], name=f"dequant_w{l}"))
            bname = None
            if L["bias_q"] is not None and not weight_only:
                inits.append(tensor(f"B{l}", L["bias_q"].astype(np.int32), int32_data=int32_data))
                bs = L["bias_scale"]
                inits.append(tensor(f"B{l}_scale", bs.astype(np.float32) if bs.size > 1 else np.array(bs.reshape(-1)[0], np.float32)))
                inits.append(tensor(f"B{l}_zp", np.zeros(bs.shape if bs.size > 1 else (), np.int32)))
                nodes.append(node("DequantizeLinear", [f"B{l}", f"B{l}_scale", f"B{l}_zp"], [f"B{l}_dq"], [attr_i("axis", 0)], name=f"dequant_b{l}"))
                bname = f"B{l}_dq"
            elif L["bias_q"] is not None or L["bias_f"] is not None:
                bf = L["bias_f"] if L["bias_f"] is not None else (L["bias_q"] * np.broadcast_to(L["bias_scale"], (m,))).astype(np.float32)
                inits.append(tensor(f"B{l}", bf.astype(np.float32)))
                bname = f"B{l}"
            z = f"Z{l}"
            if layer == "matmul_add":
                nodes.append(node("MatMul", [cur, f"W{l}_dq"], [z if bname else f"ZB{l}"], name=f"matmul{l}"))
                if bname:
                    nodes.append(node("Add", [z, bname], [f"ZB{l}"], name=f"add{l}"))
            else:
                nodes.append(node("Gemm", [cur, f"W{l}_dq"] + ([bname] if bname else []), [f"ZB{l}"], [attr_i("transB", 1)] if trans else [], name=f"gemm{l}"))
            cur = f"ZB{l}"
            if acts[l] == "Relu":
                nodes.append(node("Relu", [cur], [f"A{l}"], name=f"relu{l}"))
                cur = f"A{l}"
            elif acts[l]:
                inits += [tensor(f"clip{l}_lo", np.array(acts[l][1], np.float32)), tensor(f"clip{l}_hi", np.array(acts[l][2], np.float32))]
                nodes.append(node("Clip", [cur, f"clip{l}_lo", f"clip{l}_hi"], [f"A{l}"], name=f"clip{l}"))
                cur = f"A{l}"
            if not weight_only:
                last = l == len(layers) - 1
                cur = fake_quant(cur, l + 1, ("Yf" if spec["tail"] else "Y") if last else f"H{l}")
        if weight_only and not spec["tail"]:
            nodes.append(node("Identity", [cur], ["Y"]))
    if spec["tail"]:
        nodes.append(node(spec["tail"], [cur], ["Y"], [attr_i("axis", 1)] if spec["tail"] == "Softmax" else [], name="tail"))
    return model("qmlp_" + "x".join(map(str, dims)), nodes, inits, [value_info("X", [batch, max(window, 1) * dims[0]])],
                 [value_info("Y", [batch] + ([window] if window else []) + [dims[-1]])], opset=13)


def _tail_reference(h, tail):
    if tail == "Sigmoid":
        return 1.0 / (1.0 + np.exp(-h))
    if tail == "Softmax":
        e = np.exp(h - h.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return h


def quantized_reference(spec: dict, x: np.ndarray, mode: str = "int", weight_only: bool = False, tail: bool = True) -> np.ndarray:
    """What a quantized_mlp_spec network computes on x.  "int": the QDense definition layer by layer -- f32
    scalars, an int64 accumulator; "f64" / "f32": the QDQ graph evaluated in that float type.  The tail (Sigmoid / Softmax) is applied
    in float64 in "int" and "f64" mode.  weight_only: the graph with only its weights quantised (float modes)."""
    f32 = np.float32
    qmin, qmax = _qrange(spec["x_type"])
    layers, q, acts = spec["layers"], spec["q"], spec["acts"]
    if mode == "int":
        h = np.asarray(x, f32)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for l, L in enumerate(layers):
                xs, xz = f32(q[l][0]), q[l][1]
                ys, yz = f32(q[l + 1][0]), q[l + 1][1]
                xq = np.clip(np.rint(h / xs) + f32(xz), f32(qmin), f32(qmax)).astype(np.int64)
                acc = (xq - xz) @ (L["wq"] - L["w_zp"][None, :])
                if L["bias_q"] is not None:
                    acc = acc + L["bias_q"][None, :]
                assert np.abs(acc).max(initial=0) < 2 ** 31
                mult = (xs * L["w_scale"]).astype(f32)
                real = acc.astype(f32) * mult[None, :]
                if L["bias_f"] is not None:
                    real = (real + L["bias_f"][None, :].astype(f32)).astype(f32)
                real = _float_act(real, acts[l]).astype(f32)
                qq = np.clip(np.rint(real / ys) + f32(yz), f32(qmin), f32(qmax))
                h = ((qq - f32(yz)) * ys).astype(f32)
        return _tail_reference(h.astype(np.float64), spec["tail"]).astype(f32) if tail and spec["tail"] else h
    ft = np.float64 if mode == "f64" else f32
    assert mode in ("f64", "f32")

    def fq(h, i):
        s, z = ft(q[i][0]), ft(q[i][1])
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            return ((np.clip(np.rint(h / s) + z, ft(qmin), ft(qmax)) - z) * s).astype(ft)
    h = np.asarray(x, f32).astype(ft)
    if not weight_only:
        h = fq(h, 0)
    for l, L in enumerate(layers):
        w = ((L["wq"] - L["w_zp"][None, :]).astype(ft) * L["w_scale"].astype(ft)[None, :]).astype(ft)
        h = (h @ w).astype(ft)
        if L["bias_q"] is not None:
            h = (h + (L["bias_q"].astype(ft) * np.broadcast_to(L["bias_scale"], L["bias_q"].shape).astype(ft))[None, :]).astype(ft)
        elif L["bias_f"] is not None:
            h = (h + L["bias_f"].astype(ft)[None, :]).astype(ft)
        h = _float_act(h, acts[l]).astype(ft)
        if not weight_only:
            h = fq(h, l + 1)
    if tail and spec["tail"]:
        h = _tail_reference(h.astype(np.float64) if mode == "f64" else h, spec["tail"])
    return h.astype(f32)


# ------------------------------------------------------------------------------------------
# statically quantised convolutional nets (QDQ and QLinearConv spellings) and their numpy references
# ------------------------------------------------------------------------------------------

def _conv_taps(x, w, strides, pads, dilations, groups, fill):
    """sum over (c, ky, kx) of x[n, c, oh * sh - pt + ky * dh, ...] * w[m, c, ky, kx], `fill` in the padding; x [N,C,H,W], w [M,C/g,kh,kw],
    in the dtype of x (int64: exact)."""
    n, c, h, wd = x.shape
    m, cg, kh, kw = w.shape
    (sh, sw), (pt, pl, pb, pr), (dh, dw) = strides, pads, dilations
    xp = np.full((n, c, h + pt + pb, wd + pl + pr), fill, x.dtype)
    xp[:, :, pt:pt + h, pl:pl + wd] = x
    oh = (h + pt + pb - (dh * (kh - 1) + 1)) // sh + 1
    ow = (wd + pl + pr - (dw * (kw - 1) + 1)) // sw + 1
    out = np.zeros((n, m, oh, ow), x.dtype)
    mg = m // groups
    for g in range(groups):
        for ky in range(kh):
            for kx in range(kw):
                xs = xp[:, g * cg:(g + 1) * cg, ky * dh:ky * dh + (oh - 1) * sh + 1:sh, kx * dw:kx * dw + (ow - 1) * sw + 1:sw]
                out[:, g * mg:(g + 1) * mg] += np.einsum("nchw,mc->nmhw", xs, w[g * mg:(g + 1) * mg, :, ky, kx], optimize=True)
    return out


def _max_pool(x, k, s, p):
    n, c, h, wd = x.shape
    xp = np.full((n, c, h + 2 * p, wd + 2 * p), -np.inf, x.dtype)
    xp[:, :, p:p + h, p:p + wd] = x
    oh, ow = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
    out = np.full((n, c, oh, ow), -np.inf, x.dtype)
    for ky in range(k):
        for kx in range(k):
            out = np.maximum(out, xp[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s])
    return out


class _QConvBuilder:
    """Builds the op list of a quantized_conv_spec while it runs the float network on the calibration images (ranges -> scales)."""

    def __init__(self, in_shape, x_type, w_type, per_channel, w_zero_points, seed, calib_rows, x_zero_point=None, x_range=1.0):
        from .synth import table
        self.x_type, self.w_type, self.per_channel, self.w_zero_points = x_type, w_type, per_channel, w_zero_points
        self.ws = _WeightStream(seed)
        self.one_d = len(in_shape) == 2
        shape4 = (in_shape[0], 1, in_shape[1]) if self.one_d else tuple(in_shape)
        h = (x_range * table(seed + 1, 0, calib_rows, int(np.prod(in_shape)))).astype(np.float64).reshape((calib_rows,) + shape4)
        q = _calibrate(h.min(), h.max(), x_type)
        if x_zero_point is not None:
            q = (q[0], int(x_zero_point))
        self.val = {"X": h}   # float activations of the calibration images
        self.q = {"X": q}     # (scale, zero point) of every value
        self.ops = []
        self.in_shape = list(in_shape)

    def _quant_weights(self, w):
        """w [M, ...] float64 -> wq, w_scale[M or 1], w_zp[M or 1] (per output channel = axis 0)"""
        wmin, wmax = _qrange(self.w_type)
        rows = w.reshape(w.shape[0], -1) if self.per_channel else w.reshape(1, -1)
        if self.w_zero_points:
            lo, hi = np.minimum(rows.min(1), 0), np.maximum(rows.max(1), 0)
            w_scale = (np.maximum(hi - lo, 1e-6) / (wmax - wmin)).astype(np.float32)
            w_zp = np.clip(np.rint(wmin - lo / w_scale), wmin, wmax).astype(np.int64)
        else:
            w_scale = (np.maximum(np.abs(rows).max(1), 1e-6) / 127.0).astype(np.float32)
            w_zp = np.full(w_scale.shape, 0 if self.w_type == "int8" else 128, np.int64)
        bshape = (-1,) + (1,) * (w.ndim - 1)
        wq = np.clip(np.rint(w / w_scale.astype(np.float64).reshape(bshape)) + w_zp.reshape(bshape), wmin, wmax).astype(np.int64)
        return wq, w_scale, w_zp

    def _bias(self, op, b, xs, bias):
        m = b.shape[0]
        op["bias_q"] = op["bias_f"] = None
        if bias == "int32":
            op["bias_scale"] = (np.float32(xs) * op["w_scale"]).astype(np.float32)  # the f32 product, as the loader forms it
            op["bias_q"] = np.rint(b / np.broadcast_to(op["bias_scale"].astype(np.float64), (m,))).astype(np.int64)
            return op["bias_q"] * np.broadcast_to(op["bias_scale"].astype(np.float64), (m,))
        if bias == "f32":
            op["bias_f"] = b.astype(np.float32)
            return op["bias_f"].astype(np.float64)
        return np.zeros(m)

    def conv(self, src, out, m, k, stride=1, pads=0, dilation=1, groups=1, act="", bias="int32", weights=None):
        h = self.val[src]
        c = h.shape[1]
        kh, kw = (1, k) if self.one_d and np.isscalar(k) else ((k, k) if np.isscalar(k) else tuple(k))
        pair = lambda v: (1, v) if self.one_d and np.isscalar(v) else ((v, v) if np.isscalar(v) else tuple(v))  # noqa: E731
        strides, dil = pair(stride), pair(dilation)
        pads = (0, pads, 0, pads) if self.one_d and np.isscalar(pads) else ((pads,) * 4 if np.isscalar(pads) else tuple(pads))
        fan = c // groups * kh * kw
        if weights is None:
            w = self.ws.take((m, c // groups, kh, kw), fan).astype(np.float64)
            b = self.ws.take((m,), fan).astype(np.float64)
        else:
            w, b = (np.asarray(a, np.float64) for a in weights)
        wq, w_scale, w_zp = self._quant_weights(w)
        op = {"op": "conv", "in": src, "out": out, "wq": wq, "w_scale": w_scale, "w_zp": w_zp, "strides": strides, "pads": pads, "dilations": dil,
              "group": groups, "act": act}
        bf = self._bias(op, b, self.q[src][0], bias)
        bshape = (-1, 1, 1, 1)
        wd = (wq - w_zp.reshape(bshape)) * w_scale.astype(np.float64).reshape(bshape)
        y = _float_act(_conv_taps(h, wd, strides, pads, dil, groups, 0.0) + bf.reshape(1, -1, 1, 1), act)
        self._finish(op, out, y)

    def _finish(self, op, out, y):
        self.val[out] = y
        self.q[out] = _calibrate(y.min(), y.max(), self.x_type)
        self.ops.append(op)

    def maxpool(self, src, out, k, s, p):
        self.val[out], self.q[out] = _max_pool(self.val[src], k, s, p), self.q[src]
        self.ops.append({"op": "maxpool", "in": src, "out": out, "k": k, "s": s, "p": p})

    def add(self, a, b, out, act="Relu"):
        self._finish({"op": "add", "in": [a, b], "out": out, "act": act}, out, _float_act(self.val[a] + self.val[b], act))

    def gmaxpool(self, src, out):
        self.val[out], self.q[out] = self.val[src].max(axis=(2, 3)), self.q[src]
        self.ops.append({"op": "gmaxpool", "in": src, "out": out})

    def gemm(self, src, out, m):
        h = self.val[src]
        k = h.shape[1]
        w = self.ws.take((m, k), k).astype(np.float64)
        wq, w_scale, w_zp = self._quant_weights(w)
        op = {"op": "gemm", "in": src, "out": out, "wq": wq, "w_scale": w_scale, "w_zp": w_zp, "bias_q": None, "bias_f": None, "act": ""}
        self._finish(op, out, h @ ((wq - w_zp[:, None]) * w_scale.astype(np.float64)[:, None]).T)

    def spec(self, name):
        out = self.ops[-1]["out"]
        shape = list(self.val[out].shape[1:])
        if self.one_d and len(shape) == 3:
            shape = [shape[0], shape[2]]
        return {"name": name, "x_type": self.x_type, "w_type": self.w_type, "per_channel": self.per_channel, "in_shape": self.in_shape, "out_shape": shape,
                "ops": self.ops, "q": self.q, "out": out}


def quantized_conv_spec(kind: str = "layer", in_shape: Sequence[int] = (3, 9, 9), m: int = 8, k=3, stride=1, pads=0, dilation=1, groups: int = 1, act="Relu",
                        bias: str | None = "int32", pooled: bool = False, x_type: str = "uint8", w_type: str = "int8", per_channel: bool = True,
                        w_zero_points: bool = False, x_zero_point: int | None = None, seed: int = 1234, calib_rows: int = 4, width: int = 8,
                        classes: int = 10, x_range: float = 1.0) -> dict:
    """A convolutional net quantised the way ONNX Runtime's quantize_static does (weights per tensor or per output channel, activations
    per tensor from the float net's ranges on `calib_rows` images of the synthetic table).
    kind "layer": ONE convolution [N] + in_shape ([C,H,W], or [C,L]: Conv1d) -> m channels (k, stride, pads, dilation: a number or one
      per axis, pads (top, left, bottom, right)); pooled: GlobalMaxPool -> Flatten behind it (the served output is [N, m]).
    kind "resnet": stem conv -> MaxPool 3x3/2 -> two basic blocks (the second with stride 2 and a 1x1 projection) -> GlobalMaxPool ->
      Flatten -> Gemm; `width` channels, 2 * width after the second block.
    kind "resnet18": the topology of resnet18() with BatchNormalization folded into the convolutions (as quantisers do first) and a
      global MAX pool, `width` channels in the first stage.
    spec["ops"]: the operations in order; spec["q"][name] = (scale, zero point) of every value."""
    assert x_type in ("int8", "uint8") and w_type in ("int8", "uint8") and bias in ("int32", "f32", None)
    b = _QConvBuilder(in_shape, x_type, w_type, per_channel, w_zero_points, seed, calib_rows, x_zero_point, x_range)
    if kind == "layer":
        b.conv("X", "C0", m, k, stride, pads, dilation, groups, act, bias)
        if pooled:
            b.gmaxpool("C0", "P0")
        return b.spec("qconv_layer")
    assert len(in_shape) == 3

    def block(x, cout, stride, tag):
        cin = b.val[x].shape[1]
        b.conv(x, tag + "a", cout, 3, stride, 1, act="Relu")
        b.conv(tag + "a", tag + "b", cout, 3, 1, 1, act="")
        sc = x
        if stride != 1 or cin != cout:
            b.conv(x, tag + "p", cout, 1, stride, 0, act="")
            sc = tag + "p"
        b.add(tag + "b", sc, tag)
        return tag

    if kind == "resnet":
        b.conv("X", "stem", width, 3, 1, 1, act="Relu")
        b.maxpool("stem", "pool", 3, 2, 1)
        x = block(block("pool", width, 1, "b1"), 2 * width, 2, "b2")
    else:
        assert kind == "resnet18"
        ws, eps = b.ws, 1e-5
        orig_conv = b.conv

        def conv_bn(src, out, mo, kk, stride=1, pads=0, dilation=1, groups=1, act="", bias="int32", weights=None):  # resnet18()'s stream, folded
            cin = b.val[src].shape[1]
            w = ws.take((mo, cin, kk, kk), cin * kk * kk).astype(np.float64)
            scale, beta, mean = 1.0 + 0.1 * ws.take((mo,), 1), 0.1 * ws.take((mo,), 1), 0.1 * ws.take((mo,), 1)
            var = 1.0 + 0.5 * np.abs(ws.take((mo,), 1))
            f = scale.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)
            orig_conv(src, out, mo, kk, stride, pads, act=act, weights=(w * f[:, None, None, None], beta - mean * f))
        b.conv = conv_bn
        b.conv("X", "stem", width, 7, 2, 3, act="Relu")
        b.maxpool("stem", "pool", 3, 2, 1)
        x, i = "pool", 0
        for stage, cout in enumerate([width, width * 2, width * 4, width * 8]):
            for blk in range(2):
                i += 1
                x = block(x, cout, 2 if (stage > 0 and blk == 0) else 1, f"b{i}")
    b.gmaxpool(x, "gp")
    b.gemm("gp", "fc", classes)
    return b.spec("qconv_" + kind)


def quantized_conv_from_spec(spec: dict, form: str = "qdq", weight_only: bool = False, batch: int | str = "N") -> bytes:
    """A quantized_conv_spec net as a QDQ graph (QuantizeLinear / DequantizeLinear around float Conv / MaxPool / Add / Gemm nodes) or in the
    QOperator spelling (form="qlinear": QLinearConv / QLinearMatMul on quantised tensors; MaxPool, the residual Add and the global pool
    between DequantizeLinear and QuantizeLinear; an int32 bias or none, and only activations the output range already applies).
    weight_only (QDQ): only the weights are quantised."""
    xt, wt = _np_qtype(spec["x_type"]), _np_qtype(spec["w_type"])
    qmin = _qrange(spec["x_type"])[0]
    q = spec["q"]
    nodes, inits, made = [], [], set()
    one_d = len(spec["in_shape"]) == 2
    fname, qname = {"X": "X"}, {}   # value -> the float tensor / the quantised tensor that holds it

    def const(name, arr):
        if name not in made:
            made.add(name)
            inits.append(tensor(name, arr))
        return name

    def qparams(v):
        return const(f"{v}_scale", np.array(q[v][0], np.float32)), const(f"{v}_zp", np.array(q[v][1], xt))

    def quantise(v):  # the quantised tensor of value v
        if v not in qname:
            nodes.append(node("QuantizeLinear", [fname[v], *qparams(v)], [f"{v}_q"], name=f"quant_{v}"))
            qname[v] = f"{v}_q"
        return qname[v]

    def dequantise(v, raw=None):  # the float tensor of value v (raw: the float tensor BEFORE its quantisation)
        if raw is not None:
            fname[v] = raw
            if weight_only:
                return raw
            qname.pop(v, None)
            del fname[v]
            nodes.append(node("QuantizeLinear", [raw, *qparams(v)], [f"{v}_q"], name=f"quant_{v}"))
            qname[v] = f"{v}_q"
        if v not in fname:
            nodes.append(node("DequantizeLinear", [qname[v], *qparams(v)], [f"{v}_dq"], name=f"dequant_{v}"))
            fname[v] = f"{v}_dq"
        return fname[v]

    def wparams(o, op):
        pc = spec["per_channel"]
        return (const(f"{o}_w_scale", op["w_scale"].astype(np.float32) if pc else np.array(op["w_scale"][0], np.float32)),
                const(f"{o}_w_zp", op["w_zp"].astype(wt) if pc else np.array(op["w_zp"][0], wt)))

    def conv_attrs(op):
        if one_d:
            return [attr_ints("kernel_shape", [op["wq"].shape[3]]), attr_ints("strides", [op["strides"][1]]), attr_ints("pads", [op["pads"][1], op["pads"][3]]),
                    attr_ints("dilations", [op["dilations"][1]]), attr_i("group", op["group"])]
        return [attr_ints("kernel_shape", list(op["wq"].shape[2:])), attr_ints("strides", list(op["strides"])), attr_ints("pads", list(op["pads"])),
                attr_ints("dilations", list(op["dilations"])), attr_i("group", op["group"])]

    def activation(op, cur, o):
        if op["act"] == "Relu":
            nodes.append(node("Relu", [cur], [f"{o}_act"], name=f"relu_{o}"))
            return f"{o}_act"
        if op["act"]:
            lo, hi = const(f"{o}_lo", np.array(op["act"][1], np.float32)), const(f"{o}_hi", np.array(op["act"][2], np.float32))
            nodes.append(node("Clip", [cur, lo, hi], [f"{o}_act"], name=f"clip_{o}"))
            return f"{o}_act"
        return cur

    if form == "qdq" and not weight_only:
        dequantise("X", raw="X")
    for op in spec["ops"]:
        o, kind = op["out"], op["op"]
        if kind in ("conv", "gemm"):
            wq = op["wq"][:, :, 0, :] if one_d and kind == "conv" else op["wq"]
            if form == "qlinear":
                if op["bias_f"] is not None:
                    raise ValueError("QLinearConv carries an int32 bias")
                if op["act"] and not (op["act"] == "Relu" and q[o][1] == qmin):
                    raise ValueError("the QLinear spelling cannot express activation %r before zero point %d" % (op["act"], q[o][1]))
                src = op["in"]
                xq = quantise(src)
                if kind == "conv":
                    ins = [xq, *qparams(src), const(f"{o}_w", wq.astype(wt)), *wparams(o, op), *qparams(o)]
                    if op["bias_q"] is not None:
                        ins.append(const(f"{o}_b", op["bias_q"].astype(np.int32)))
                    nodes.append(node("QLinearConv", ins, [f"{o}_q"], conv_attrs(op), name=f"qconv_{o}"))
                else:
                    ins = [xq, *qparams(src), const(f"{o}_w", np.ascontiguousarray(wq.T).astype(wt)), *wparams(o, op), *qparams(o)]
                    nodes.append(node("QLinearMatMul", ins, [f"{o}_q"], name=f"qmm_{o}"))
                qname[o] = f"{o}_q"
                continue
            src = dequantise(op["in"])
            ws_, wz_ = wparams(o, op)
            nodes.append(node("DequantizeLinear", [const(f"{o}_w", wq.astype(wt)), ws_, wz_], [f"{o}_w_dq"], [attr_i("axis", 0)], name=f"dequant_w_{o}"))
            ins = [src, f"{o}_w_dq"]
            if op["bias_q"] is not None and not weight_only:
                bs = op["bias_scale"]
                const(f"{o}_b_scale", bs.astype(np.float32) if bs.size > 1 else np.array(bs.reshape(-1)[0], np.float32))
                const(f"{o}_b_zp", np.zeros(bs.shape if bs.size > 1 else (), np.int32))
                nodes.append(node("DequantizeLinear", [const(f"{o}_b", op["bias_q"].astype(np.int32)), f"{o}_b_scale", f"{o}_b_zp"], [f"{o}_b_dq"],
                                  [attr_i("axis", 0)], name=f"dequant_b_{o}"))
                ins.append(f"{o}_b_dq")
            elif op["bias_q"] is not None or op["bias_f"] is not None:
                bf = op["bias_f"] if op["bias_f"] is not None else (op["bias_q"] * np.broadcast_to(op["bias_scale"], op["bias_q"].shape)).astype(np.float32)
                ins.append(const(f"{o}_b", bf.astype(np.float32)))
            if kind == "conv":
                nodes.append(node("Conv", ins, [f"{o}_raw"], conv_attrs(op), name=f"conv_{o}"))
            else:
                nodes.append(node("Gemm", ins, [f"{o}_raw"], [attr_i("transB", 1)], name=f"gemm_{o}"))
            dequantise(o, raw=activation(op, f"{o}_raw", o))
        elif kind == "maxpool":
            nodes.append(node("MaxPool", [dequantise(op["in"])], [f"{o}_raw"], [attr_ints("kernel_shape", [op["k"]] * 2), attr_ints("strides", [op["s"]] * 2),
                                                                               attr_ints("pads", [op["p"]] * 4)], name=f"pool_{o}"))
            if form == "qdq":
                dequantise(o, raw=f"{o}_raw")
            else:
                fname[o] = f"{o}_raw"
        elif kind == "add":
            nodes.append(node("Add", [dequantise(op["in"][0]), dequantise(op["in"][1])], [f"{o}_sum"], name=f"add_{o}"))
            raw = activation(op, f"{o}_sum", o)
            if form == "qdq":
                dequantise(o, raw=raw)
            else:
                fname[o] = raw
                quantise(o)
                del fname[o]
        elif kind == "gmaxpool":
            nodes.append(node("GlobalMaxPool", [dequantise(op["in"])], [f"{o}_gp"], name=f"gpool_{o}"))
            nodes.append(node("Flatten", [f"{o}_gp"], [f"{o}_flat"], [attr_i("axis", 1)], name=f"flatten_{o}"))
            fname[o] = f"{o}_flat"
            if form == "qdq" and o != spec["out"]:
                dequantise(o, raw=f"{o}_flat")
    nodes.append(node("Identity", [dequantise(spec["out"])], ["Y"], name="served"))
    return model(spec["name"], nodes, inits, [value_info("X", [batch] + list(spec["in_shape"]))], [value_info("Y", [batch] + list(spec["out_shape"]))], opset=13)


def quantized_conv_reference(spec: dict, x: np.ndarray, mode: str = "int", weight_only: bool = False) -> np.ndarray:
    """What a quantized_conv_spec net computes on x [N] + in_shape.  "int": the QConv2d / QDense definition step by
    step -- f32 scalars, an int64 accumulator checked to fit int32, padding = the zero point, the residual Add one f32 addition of two
    dequantised values followed by its FakeQuant; grouped convolutions in float32 on the dequantised values (their float fallback).
    "f64": the QDQ graph evaluated in float64 (weight_only: with only its weights quantised)."""
    f32 = np.float32
    qmin, qmax = _qrange(spec["x_type"])
    q = spec["q"]
    one_d = len(spec["in_shape"]) == 2
    x = np.asarray(x, f32)
    x = x.reshape((x.shape[0],) + ((spec["in_shape"][0], 1, spec["in_shape"][1]) if one_d else tuple(spec["in_shape"])))
    ft = f32 if mode == "int" else np.float64
    assert mode in ("int", "f64")

    def fq(h, v):
        if weight_only:
            return h
        s, z = ft(q[v][0]), ft(q[v][1])
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            return ((np.clip(np.rint(h / s) + z, ft(qmin), ft(qmax)) - z) * s).astype(ft)

    def bshape(op):
        return (1, -1, 1, 1) if op["op"] == "conv" else (1, -1)

    def float_layer(op, h):
        wb = (-1, 1, 1, 1) if op["op"] == "conv" else (-1, 1)
        w = ((op["wq"] - op["w_zp"].reshape(wb)).astype(ft) * op["w_scale"].astype(ft).reshape(wb)).astype(ft)
        y = _conv_taps(h, w, op["strides"], op["pads"], op["dilations"], op["group"], ft(0)) if op["op"] == "conv" else (h @ w.T).astype(ft)
        if op["bias_q"] is not None:
            y = (y + (op["bias_q"].astype(ft) * np.broadcast_to(op["bias_scale"], op["bias_q"].shape).astype(ft)).reshape(bshape(op))).astype(ft)
        elif op["bias_f"] is not None:
            y = (y + op["bias_f"].astype(ft).reshape(bshape(op))).astype(ft)
        return _float_act(y, op["act"]).astype(ft)

    def int_layer(op, h):
        src, o = op["in"], op["out"]
        xs, xz, ys, yz = f32(q[src][0]), q[src][1], f32(q[o][0]), q[o][1]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            xq = np.clip(np.rint(h / xs) + f32(xz), f32(qmin), f32(qmax)).astype(np.int64)
            wb = (-1, 1, 1, 1) if op["op"] == "conv" else (-1, 1)
            wz = op["wq"] - op["w_zp"].reshape(wb)
            acc = _conv_taps(xq - xz, wz, op["strides"], op["pads"], op["dilations"], 1, 0) if op["op"] == "conv" else (xq - xz) @ wz.T
            if op["bias_q"] is not None:
                acc = acc + op["bias_q"].reshape(bshape(op))
            assert np.abs(acc).max(initial=0) < 2 ** 31
            real = acc.astype(f32) * (xs * op["w_scale"]).astype(f32).reshape(bshape(op))
            if op["bias_f"] is not None:
                real = (real + op["bias_f"].astype(f32).reshape(bshape(op))).astype(f32)
            real = _float_act(real, op["act"]).astype(f32)
            qq = np.clip(np.rint(real / ys) + f32(yz), f32(qmin), f32(qmax))
            return ((qq - f32(yz)) * ys).astype(f32)

    val = {"X": x if mode == "int" else fq(x.astype(ft), "X")}
    for op in spec["ops"]:
        o, kind = op["out"], op["op"]
        if kind in ("conv", "gemm"):
            h = val[op["in"]]
            if mode == "int" and (kind == "gemm" or op["group"] == 1):
                val[o] = int_layer(op, h)
            else:  # (in "int" mode: a grouped layer's float fallback, on the values its input quantisation leaves)
                val[o] = fq(float_layer(op, fq(h, op["in"]) if mode == "int" else h), o)
        elif kind == "maxpool":
            val[o] = _max_pool(val[op["in"]], op["k"], op["s"], op["p"])
        elif kind == "add":
            val[o] = fq(_float_act((val[op["in"][0]] + val[op["in"][1]]).astype(ft), op["act"]).astype(ft), o)
        elif kind == "gmaxpool":
            val[o] = val[op["in"]].max(axis=(2, 3))
    out = val[spec["out"]].astype(f32)
    return out.reshape((out.shape[0],) + tuple(spec["out_shape"]))


# ------------------------------------------------------------------------------------------
# float16 models: half MLPs and a small half CNN, their exact numpy references and derived bounds
# ------------------------------------------------------------------------------------------
_f16, _f64 = np.float16, np.float64


def _h(v):
    """v rounded once to IEEE half (numpy's astype: nearest even), as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(v).astype(_f16).astype(_f64)


def _half_act(r, act):
    """act(r) for half values r (float64), BEFORE its rounding to half.  LeakyRelu multiplies in f32, as the device does (alpha is an f32
    attribute: the f32 product rounded to half is the definition); the others are evaluated in float64."""
    if not act:
        return r
    kind = act[0]
    if kind == "Relu":
        return np.maximum(r, 0.0)
    if kind == "LeakyRelu":
        return np.where(r >= 0, r, (np.float32(act[1]) * r.astype(np.float32)).astype(_f64))
    if kind == "Clip":
        return np.minimum(np.maximum(r, _f64(_f16(act[1]))), _f64(_f16(act[2])))
    if kind == "Sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-r))
    if kind == "Tanh":
        return np.tanh(r)
    raise ValueError(kind)


def _as_act(a):
    return None if not a else ((a,) if isinstance(a, str) else tuple(a))


def half_mlp_spec(dims: Sequence[int] = (128, 256, 64, 1), act="Relu", tail: str = "", seed: int = 1234, grid: bool = False, bias: bool = True,
                  acts: Sequence | None = None) -> dict:
    """A float16 MLP: layers[l] = {w [K, M] float16, b [M] float16 | None, act}.  `act` follows every layer but the last (acts: one per
    layer instead); an act is "Relu" | "Sigmoid" | "Tanh" | ("LeakyRelu", alpha) | ("Clip", lo, hi).  Generic: weights and biases uniform
    in +-1/sqrt(K), rounded to half.  grid=True: weights and biases are multiples of 1/2 in [-1, 1] and inputs (half_inputs) multiples of
    1/8, so every product of layer l is a multiple of spec["q"][l] and sums below 2^24 q are exact in f32 in any order."""
    n = len(dims) - 1
    acts = [_as_act(a) for a in (acts if acts is not None else [act] * (n - 1) + [None])]
    rng = np.random.default_rng(seed)
    layers, q, q_in = [], [], 0.125
    for l in range(n):
        K, M = int(dims[l]), int(dims[l + 1])
        if grid:
            w = (rng.integers(-2, 3, size=(K, M)) / 2.0).astype(_f16)
            b = (rng.integers(-2, 3, size=M) / 2.0).astype(_f16) if bias else None
        else:
            w = (rng.uniform(-1, 1, size=(K, M)) / math.sqrt(K)).astype(_f16)
            b = (rng.uniform(-1, 1, size=M) / math.sqrt(K)).astype(_f16) if bias else None
        layers.append({"w": w, "b": b, "act": acts[l]})
        q.append(q_in * 0.5)
        q_in = q[-1] * (float(acts[l][1]) if acts[l] and acts[l][0] == "LeakyRelu" else 1.0)
    return {"dims": tuple(int(d) for d in dims), "layers": layers, "tail": tail, "grid": grid, "q": q if grid else None, "seed": seed}


def half_inputs(spec: dict, rows: int, seed: int = 0) -> np.ndarray:
    """f32 inputs [rows, K0]: multiples of 1/8 in [-1, 1] for a grid spec, standard normal values else."""
    rng = np.random.default_rng(1000 + seed)
    k = spec["dims"][0] if "dims" in spec else int(np.prod(spec["in_shape"]))
    if spec["grid"]:
        return (rng.integers(-8, 9, size=(rows, k)) / 8.0).astype(np.float32)
    return rng.standard_normal((rows, k)).astype(np.float32)


def _half_act_nodes(nodes, inits, act, src, dst, name):
    kind = act[0]
    if kind == "LeakyRelu":
        nodes.append(node("LeakyRelu", [src], [dst], [attr_f("alpha", float(act[1]))], name=name))
    elif kind == "Clip":
        inits.append(tensor(name + "_lo", np.array(act[1], _f16)))
        inits.append(tensor(name + "_hi", np.array(act[2], _f16)))
        nodes.append(node("Clip", [src, name + "_lo", name + "_hi"], [dst], name=name))
    else:
        nodes.append(node(kind, [src], [dst], name=name))


def half_from_spec(spec: dict, io: str = "float", spelling: str = "gemm", int32_data: bool = False, alpha: float = 1.0, layer_outputs: bool = False,
                   window: int = 0) -> bytes:
    """The ONNX model of a half_mlp_spec.  io="float": float input and output around Cast nodes (what keep_io_types produces);
    "half": float16 graph input and output.  spelling: Gemm, or MatMul -> Add.  layer_outputs: every layer's result is a graph output too
    ("h0", "h1", ...; served through name#output).  window = T > 0: the input is [N, T, K] and the MatMul spelling runs per time step."""
    dims = spec["dims"]
    nodes, inits, outs = [], [], []
    t_io = FLOAT if io == "float" else FLOAT16
    in_dims = ["N", window, dims[0]] if window else ["N", dims[0]]
    cur = "X"
    if io == "float":
        nodes.append(node("Cast", ["X"], ["x_h"], [attr_i("to", FLOAT16)], name="cast_in"))
        cur = "x_h"
    for l, L in enumerate(spec["layers"]):
        inits.append(tensor(f"W{l}", L["w"], int32_data=int32_data))
        if L["b"] is not None:
            inits.append(tensor(f"B{l}", L["b"], int32_data=int32_data))
        out = f"d{l}"
        if spelling == "gemm" and not window:
            attrs = [attr_f("alpha", alpha)] if alpha != 1.0 else []
            nodes.append(node("Gemm", [cur, f"W{l}"] + ([f"B{l}"] if L["b"] is not None else []), [out], attrs, name=f"gemm{l}"))
        else:
            nodes.append(node("MatMul", [cur, f"W{l}"], [f"m{l}" if L["b"] is not None else out], name=f"matmul{l}"))
            if L["b"] is not None:
                nodes.append(node("Add", [f"m{l}", f"B{l}"], [out], name=f"add{l}"))
        cur = out
        if L["act"]:
            _half_act_nodes(nodes, inits, L["act"], cur, f"a{l}", f"act{l}")
            cur = f"a{l}"
        if layer_outputs:
            nodes.append(node("Identity", [cur], [f"h{l}"], name=f"tap{l}"))
            outs.append(value_info(f"h{l}", (["N", window] if window else ["N"]) + [dims[l + 1]], FLOAT16))
    if spec["tail"]:
        nodes.append(node(spec["tail"], [cur], ["t"], [attr_i("axis", -1)] if spec["tail"] == "Softmax" else [], name="tail"))
        cur = "t"
    if io == "float":
        nodes.append(node("Cast", [cur], ["Y"], [attr_i("to", FLOAT)], name="cast_out"))
    else:
        nodes.append(node("Identity", [cur], ["Y"], name="out"))
    out_dims = (["N", window] if window else ["N"]) + [dims[-1]]
    return model("half_mlp", nodes, inits, [value_info("X", in_dims, t_io)], [value_info("Y", out_dims, t_io)] + outs)


def _half_layer(L, h, spelling, S=None):
    """One layer of the definition on half values h (float64): the result before the activation's own rounding."""
    acc = h @ L["w"].astype(_f64)
    if L["b"] is None:
        return _h(acc)
    b = L["b"].astype(_f64)
    return _h(acc + b) if spelling == "gemm" else _h(_h(acc) + b)


def half_reference(spec: dict, x: np.ndarray, spelling: str = "gemm", layers: bool = False):
    """The definition of the half plan in float64: the input rounded to half, per layer r = half(acc + b) (gemm) or
    half(half(acc) + b) (matmul_add), then r = half(act(r)); a tail (Softmax, Sigmoid ...) in float64 and rounded once.  Exact on grid
    specs; on generic data the device's f32 sum differs (half_bounds).  layers=True: the list of every layer's result as well."""
    h = _h(np.asarray(x, np.float32))
    per = []
    for L in spec["layers"]:
        h = _half_layer(L, h, spelling)
        if L["act"]:
            h = _h(_half_act(h, L["act"]))
        per.append(h.astype(np.float32))
    if spec["tail"]:
        h = _h(_tail_reference(h, spec["tail"]))
    out = h.astype(np.float32)
    return (out, per) if layers else out


def half_sums(spec: dict, x: np.ndarray, spelling: str = "gemm") -> list:
    """max over rows and columns of sum_k |x_k w_k| + |b| at every layer of the reference (grid specs: compare with 2^24 q)."""
    h = _h(np.asarray(x, np.float32))
    out = []
    for L in spec["layers"]:
        S = np.abs(h) @ np.abs(L["w"].astype(_f64)) + (0 if L["b"] is None else np.abs(L["b"].astype(_f64)))
        out.append(float(S.max()))
        h = _half_layer(L, h, spelling)
        if L["act"]:
            h = _h(_half_act(h, L["act"]))
    return out


def half_bounds(spec: dict, x: np.ndarray, spelling: str = "gemm", layer: int = 0):
    """(lo, hi): float32 arrays of half values between which every element of layer `layer`'s result must lie when its input is x, for
    ANY order of the f32 sum.  With e the exact sum (+ bias for gemm), S = sum |x_k w_k| (+ |b|) and gamma = K 2^-24 the computed f32
    value lies in [e - gamma S, e + gamma S]; rounding to half and Relu / LeakyRelu / Clip are monotone, so the bounds pass through them.
    Sigmoid / Tanh: the argument interval, and 2 f32 ulps on the value for the device's exp / tanh."""
    L = spec["layers"][layer]
    h = _h(np.asarray(x, np.float32))
    w = L["w"].astype(_f64)
    K = w.shape[0]
    gamma = K * 2.0 ** -24
    e, S = h @ w, np.abs(h) @ np.abs(w)
    if L["b"] is None:
        lo, hi = _h(e - gamma * S), _h(e + gamma * S)
    elif spelling == "gemm":
        b = L["b"].astype(_f64)
        S = S + np.abs(b)
        lo, hi = _h(e + b - gamma * S), _h(e + b + gamma * S)
    else:
        b = L["b"].astype(_f64)
        lo, hi = _h(_h(e - gamma * S) + b), _h(_h(e + gamma * S) + b)
    if L["act"]:
        lo, hi = _half_act(lo, L["act"]), _half_act(hi, L["act"])
        if L["act"][0] in ("Sigmoid", "Tanh"):
            lo = lo - 2 * np.spacing(np.abs(lo).astype(np.float32)).astype(_f64)
            hi = hi + 2 * np.spacing(np.abs(hi).astype(np.float32)).astype(_f64)
        lo, hi = _h(lo), _h(hi)
    return lo.astype(np.float32), hi.astype(np.float32)


def half_cnn_spec(in_shape: Sequence[int] = (8, 9, 9), m1: int = 8, m2: int = 16, classes: int = 5, seed: int = 21, grid: bool = True) -> dict:
    """Conv3x3 -> Relu -> MaxPool 2/2 -> Conv2x2 -> Relu -> GlobalAveragePool -> Gemm in float16.  (9 x 9 -> 7 x 7 -> 3 x 3 -> 2 x 2: the
    average is over four values, exact on the grid.)"""
    rng = np.random.default_rng(seed)
    c = int(in_shape[0])

    def draw(shape, fan):
        if grid:
            return (rng.integers(-2, 3, size=shape) / 2.0).astype(_f16)
        return (rng.uniform(-1, 1, size=shape) / math.sqrt(fan)).astype(_f16)

    return {"in_shape": tuple(int(d) for d in in_shape), "grid": grid, "seed": seed,
            "w1": draw((m1, c, 3, 3), c * 9), "b1": draw((m1,), c * 9), "w2": draw((m2, m1, 2, 2), m1 * 4), "b2": draw((m2,), m1 * 4),
            "w3": draw((m2, classes), m2), "b3": draw((classes,), m2), "q": [1 / 16, 1 / 32, 1 / 256] if grid else None}


def half_cnn_from_spec(spec: dict, io: str = "float") -> bytes:
    c, hh, ww = spec["in_shape"]
    t_io = FLOAT if io == "float" else FLOAT16
    nodes, cur = [], "X"
    if io == "float":
        nodes.append(node("Cast", ["X"], ["x_h"], [attr_i("to", FLOAT16)], name="cast_in"))
        cur = "x_h"
    inits = [tensor(k.upper(), spec[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    nodes += [node("Conv", [cur, "W1", "B1"], ["c1"], [attr_ints("kernel_shape", [3, 3])], name="conv1"), node("Relu", ["c1"], ["r1"], name="relu1"),
              node("MaxPool", ["r1"], ["p1"], [attr_ints("kernel_shape", [2, 2]), attr_ints("strides", [2, 2])], name="pool1"),
              node("Conv", ["p1", "W2", "B2"], ["c2"], [attr_ints("kernel_shape", [2, 2])], name="conv2"), node("Relu", ["c2"], ["r2"], name="relu2"),
              node("GlobalAveragePool", ["r2"], ["g"], name="gap"), node("Flatten", ["g"], ["f"], [attr_i("axis", 1)], name="flatten"),
              node("Gemm", ["f", "W3", "B3"], ["d"], name="head")]
    if io == "float":
        nodes.append(node("Cast", ["d"], ["Y"], [attr_i("to", FLOAT)], name="cast_out"))
    else:
        nodes.append(node("Identity", ["d"], ["Y"], name="out"))
    return model("half_cnn", nodes, inits, [value_info("X", ["N", c, hh, ww], t_io)], [value_info("Y", ["N", spec["w3"].shape[1]], t_io)])


def half_cnn_reference(spec: dict, x: np.ndarray, sums: bool = False):
    """The half CNN in float64, every plan step's result rounded once to half (the float path's contract); sums=True: also
    max sum |x w| + |b| of the three layers."""
    n = x.shape[0]
    h = _h(np.asarray(x, np.float32)).reshape((n,) + spec["in_shape"])
    S = []

    def conv(h, w, b):
        w64, b64 = w.astype(_f64), b.astype(_f64)
        S.append(float((_conv_taps(np.abs(h), np.abs(w64), (1, 1), (0, 0, 0, 0), (1, 1), 1, 0.0) + np.abs(b64)[None, :, None, None]).max()))
        return np.maximum(_h(_conv_taps(h, w64, (1, 1), (0, 0, 0, 0), (1, 1), 1, 0.0) + b64[None, :, None, None]), 0.0)

    h = _max_pool(conv(h, spec["w1"], spec["b1"]), 2, 2, 0)
    h = _h(conv(h, spec["w2"], spec["b2"]).mean(axis=(2, 3)))
    w3, b3 = spec["w3"].astype(_f64), spec["b3"].astype(_f64)
    S.append(float((np.abs(h) @ np.abs(w3) + np.abs(b3)).max()))
    out = _h(h @ w3 + b3).astype(np.float32)
    return (out, S) if sums else out


# ------------------------------------------------------------------------------------------
# distance models (KMeans, nearest-neighbour search) and reductions along the feature axis.  skl2onnx, onnx
# and onnxruntime are not dependencies: the graphs below restate what the exporter writes for these estimators.
# ------------------------------------------------------------------------------------------

MS_DOMAIN = "com.microsoft"
NEAREST_SPELLINGS = ("gemm", "matmul_mul", "cdist")
REDUCE_OPS = ("ReduceSum", "ReduceMean", "ReduceMax", "ReduceMin", "ReduceProd", "ReduceL1", "ReduceL2", "ReduceSumSquare", "ReduceLogSum",
              "ReduceLogSumExp")


def kmeans_spec(features: int = 30, centers: int = 8, seed: int = 1234, scale: float = 1.0, offset: float = 0.0) -> dict:
    """Seeded reference set: `centers` Gaussian vectors of `features` columns (times `scale`, plus `offset`)."""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((centers, features)) * scale + offset).astype(np.float32)
    return {"features": int(features), "centers": c}


def sklearn_kmeans_spec(est) -> dict:
    """A fitted KMeans / MiniBatchKMeans (cluster_centers_) or NearestCentroid (centroids_) as a kmeans_spec()-style dict."""
    c = np.asarray(getattr(est, "cluster_centers_", getattr(est, "centroids_", None)), dtype=np.float32)
    return {"features": int(c.shape[1]), "centers": np.ascontiguousarray(c)}


def sklearn_neighbors_spec(est) -> dict:
    """A fitted NearestNeighbors / KNeighbors* (its training matrix _fit_X, Euclidean metric) as a kmeans_spec()-style dict."""
    if getattr(est, "effective_metric_", "euclidean") not in ("euclidean", "minkowski", "sqeuclidean") or getattr(est, "p", 2) not in (2, None):
        raise ValueError("only the Euclidean metric")
    c = np.asarray(est._fit_X, dtype=np.float32)
    return {"features": int(c.shape[1]), "centers": np.ascontiguousarray(c), "n_neighbors": int(getattr(est, "n_neighbors", 5))}


def _model_ms(name, nodes, inits, inputs, outputs, opset=13) -> bytes:
    return model(name, nodes, inits, inputs, outputs, opset=opset) + _ld(8, _s(1, MS_DOMAIN) + _vi(2, 1))


def _distance_nodes(spec: dict, spelling: str, x: str, out: str, c2=None, order: str = "rs_first", metric: str = "sqeuclidean"):
    """Nodes and initializers computing `out` = |x - c|^2 [N, M] in one spelling.  c2: the |c|^2 constant written into the graph (default:
    the f32 norms); order: "rs_first" (rs + g) + C2 as skl2onnx writes it, or "c2_first" rs + (C2 + g)."""
    C = np.asarray(spec["centers"], dtype=np.float32)
    M = C.shape[0]
    if spelling == "cdist":
        return [node("CDist", [x, "nn_C"], [out], [attr_s("metric", metric)], name="cdist", domain=MS_DOMAIN)], [tensor("nn_C", C)]
    if c2 is None:
        c2 = (C.astype(np.float64) ** 2).sum(1).astype(np.float32)
    inits = [tensor("nn_C2", np.asarray(c2, dtype=np.float32).reshape(1, M))]
    nodes = [node("ReduceSumSquare", [x], ["nn_rs"], [attr_ints("axes", [1]), attr_i("keepdims", 1)], name="rs")]
    if spelling == "gemm":
        inits += [tensor("nn_C", C), tensor("nn_zero", np.zeros(1, np.float32))]
        nodes.append(node("Gemm", [x, "nn_C", "nn_zero"], ["nn_g"], [attr_f("alpha", -2.0), attr_i("transB", 1)], name="gemm"))
    elif spelling == "matmul_mul":
        inits += [tensor("nn_Ct", np.ascontiguousarray(C.T)), tensor("nn_m2", np.array([-2.0], np.float32))]
        nodes += [node("MatMul", [x, "nn_Ct"], ["nn_xc"], name="matmul"), node("Mul", ["nn_xc", "nn_m2"], ["nn_g"], name="mul")]
    else:
        raise ValueError(spelling)
    if order == "rs_first":
        nodes += [node("Add", ["nn_rs", "nn_g"], ["nn_z"], name="add_rs"), node("Add", ["nn_C2", "nn_z"], [out], name="add_c2")]
    else:
        nodes += [node("Add", ["nn_g", "nn_C2"], ["nn_z"], name="add_c2"), node("Add", ["nn_z", "nn_rs"], [out], name="add_rs")]
    return nodes, inits


def kmeans_from_spec(spec: dict, spelling: str = "gemm", output: str = "label", c2=None, order: str = "rs_first", extra_reader: bool = False) -> bytes:
    """KMeans as skl2onnx writes it: outputs `label` = ArgMin(D2) [N] int64 (predict) and `scores` = Sqrt(D2) [N, M] (transform); `output`
    names the first (served by default).  extra_reader: one more graph output reads the row norms, so the sub-graph is not the pattern."""
    F, M = spec["features"], np.asarray(spec["centers"]).shape[0]
    nodes, inits = _distance_nodes(spec, spelling, "X", "nn_d2", c2=c2, order=order)
    nodes += [node("ArgMin", ["nn_d2"], ["label"], [attr_i("axis", 1), attr_i("keepdims", 0)], name="argmin"),
              node("Sqrt", ["nn_d2"], ["scores"], name="sqrt")]
    outs = [value_info("label", ["N"], INT64), value_info("scores", ["N", M])]
    if output == "scores":
        outs.reverse()
    elif output == "d2":
        outs.insert(0, value_info("nn_d2", ["N", M]))
    if extra_reader:
        outs.append(value_info("nn_rs", ["N", 1]))
    return _model_ms("kmeans", nodes, inits, [value_info("X", ["N", F])], outs)


def distance_reader_graph(spec: dict, readers: Sequence[tuple], spelling: str = "gemm") -> bytes:
    """The distance sub-graph followed by a chain of single-input `readers` -- (op, attrs) or (op, attrs, constant second input) -- whose
    last output "Y" is served: the forms exporters leave between D2 and its consumer (Identity, Flatten, Reshape ...)."""
    F, M = spec["features"], np.asarray(spec["centers"]).shape[0]
    nodes, inits = _distance_nodes(spec, spelling, "X", "nn_d2")
    src, whole = "nn_d2", False
    for n, r in enumerate(readers):
        out = "Y" if n == len(readers) - 1 else f"rd_{n}"
        ins = [src]
        if len(r) > 2:
            inits.append(tensor(f"rd_c{n}", np.asarray(r[2])))
            ins.append(f"rd_c{n}")
        nodes.append(node(r[0], ins, [out], list(r[1]), name=f"reader{n}"))
        src, whole = out, r[0] == "ArgMin"
    return _model_ms("distance_reader", nodes, inits, [value_info("X", ["N", F])], [value_info("Y", ["N"] if whole else ["N", M], INT64 if whole else FLOAT)])


def knn_search_from_spec(spec: dict, k: int = 5, output: str = "indices", spelling: str = "cdist", metric: str = "euclidean") -> bytes:
    """Nearest-neighbour SEARCH (the head of what skl2onnx writes for KNeighbors* / NearestNeighbors): TopK(largest = 0) over the
    distances; outputs `indices` [N, k] int64 and `distances` [N, k].  The gemm spellings compute squared distances and root the values."""
    F = spec["features"]
    if spelling == "cdist":
        nodes, inits = _distance_nodes(spec, spelling, "X", "nn_d", metric=metric)
        val = "distances"
    else:
        nodes, inits = _distance_nodes(spec, spelling, "X", "nn_d")
        val = "nn_v2" if metric == "euclidean" else "distances"
    inits.append(tensor("nn_k", np.array([k], np.int64)))
    nodes.append(node("TopK", ["nn_d", "nn_k"], [val, "indices"], [attr_i("axis", -1), attr_i("largest", 0), attr_i("sorted", 1)], name="topk"))
    if val != "distances":
        nodes.append(node("Sqrt", [val], ["distances"], name="sqrt_v"))
    outs = [value_info("indices", ["N", k], INT64), value_info("distances", ["N", k])]
    if output == "distances":
        outs.reverse()
    return _model_ms("knn", nodes, inits, [value_info("X", ["N", F])], outs)


def _knn_vote_front(spec: dict, y, k: int, weights: str, spelling: str, lookup: str, reshape, cast_to, eps: float, reciprocal: str, table_dtype):
    """The part the classifier and the regressor share: the search head of knn_search_from_spec (Euclidean values: CDist's own metric, or
    Sqrt on the TopK values of a gemm spelling), the lookup of `y` by the indices -> "knn_lab" [N, k] and, for weights = "distance", the
    weights "knn_wei" [N, k].  Returns (nodes, inits)."""
    if weights not in ("uniform", "distance"):
        raise ValueError(weights)
    if spelling == "cdist":
        nodes, inits = _distance_nodes(spec, spelling, "X", "nn_d", metric="euclidean")
        val = "distances"
    else:
        nodes, inits = _distance_nodes(spec, spelling, "X", "nn_d")
        val = "nn_v2"
    inits.append(tensor("nn_k", np.array([k], np.int64)))
    nodes.append(node("TopK", ["nn_d", "nn_k"], [val, "indices"], [attr_i("axis", -1), attr_i("largest", 0), attr_i("sorted", 1)], name="topk"))
    if val != "distances":
        nodes.append(node("Sqrt", [val], ["distances"], name="sqrt_v"))
    inits.append(tensor("knn_y", np.asarray(y).astype(table_dtype)))
    if lookup == "afe":  # the ai.onnx.ml operator flattens: [1, N * k]
        nodes.append(node("ArrayFeatureExtractor", ["knn_y", "indices"], ["knn_picked"], name="lookup", domain=ML_DOMAIN))
        reshape = "k" if reshape is None else reshape
    elif lookup == "gather":
        nodes.append(node("Gather", ["knn_y", "indices"], ["knn_picked"], [attr_i("axis", 0)], name="lookup"))
    else:
        raise ValueError(lookup)
    cur = "knn_picked"
    if reshape in ("k", "k1"):
        inits.append(tensor("knn_lab_shape", np.array([-1, k] if reshape == "k" else [-1, k, 1], np.int64)))
        nodes.append(node("Reshape", [cur, "knn_lab_shape"], ["knn_shaped"], name="lookup_reshape"))
        cur = "knn_shaped"
    elif reshape not in (None, "none"):
        raise ValueError(reshape)
    if cast_to is not None:
        nodes.append(node("Cast", [cur], ["knn_cast"], [attr_i("to", cast_to)], name="lookup_cast"))
        cur = "knn_cast"
    if reshape == "k1":
        inits.append(tensor("knn_sq_axes", np.array([2], np.int64)))
        nodes.append(node("Squeeze", [cur, "knn_sq_axes"], ["knn_squeezed"], name="lookup_squeeze"))
        cur = "knn_squeezed"
    lab = cur
    if weights == "distance":
        inits.append(tensor("knn_eps", np.array([eps], np.float32)))
        nodes.append(node("Max", ["distances", "knn_eps"], ["knn_clamped"], name="clamp"))
        if reciprocal == "reciprocal":
            nodes.append(node("Reciprocal", ["knn_clamped"], ["knn_wei"], name="weights"))
        elif reciprocal == "div":
            inits.append(tensor("knn_one", np.array([1.0], np.float32)))
            nodes.append(node("Div", ["knn_one", "knn_clamped"], ["knn_wei"], name="weights"))
        else:
            raise ValueError(reciprocal)
    return nodes, inits, lab


def knn_classifier_from_spec(spec: dict, y, classes, k: int = 5, weights: str = "uniform", output: str = "label", spelling: str = "cdist", zipmap: bool = False,
                             lookup: str = "afe", keepdims: int = 1, join: str = "concat", reshape=None, cast: bool = False, eps: float = 1e-6,
                             reciprocal: str = "reciprocal", final: str | None = None, also: Sequence[str] = (), equal_values=None,
                             extra_reader: str | None = None) -> bytes:
    """KNeighborsClassifier as skl2onnx writes it, restated: `y` [M] are the CLASS INDICES (0 .. C - 1) of the training rows, `classes` [C]
    the int64 class values (classes_).  Outputs `label` [N] int64 and `probabilities` [N, C]; `output` names the first (served by default).

    Recalled from the exporter's converter (convert_nearest_neighbors_classifier): the search head shared with NearestNeighbors; the
    training labels looked up by ArrayFeatureExtractor and reshaped to [-1, k]; one Equal -> Cast -> [Mul by the weights] -> ReduceSum branch
    per class joined by Concat(axis = 1); ArgMax, the class table looked up by ArrayFeatureExtractor; the probabilities as the Concat over its
    row sum; weights = "distance" as Reciprocal(Max(distances, 1e-6)); ZipMap behind the probabilities unless the zipmap option is off.
    Where the recollection is loose, the variants are parameters and the lowering recognises all of them: `lookup` ("afe" | "gather") for both
    table lookups, `keepdims` of the branch ReduceSum (0: an Unsqueeze per branch in front of the Concat, or with join = "transpose" an
    Unsqueeze(0), Concat(axis = 0) and Transpose), `reshape` of the looked-up labels (None: the lookup's natural one; "none", "k" = [-1, k],
    "k1" = [-1, k, 1] and a Squeeze), `cast` (a Cast of the labels to INT64 behind the lookup), `reciprocal` ("reciprocal" | "div" = Div(1, .)),
    `final` (what follows the class lookup: None = the lookup's natural Reshape([-1]), "none", "reshape", "cast", "reshape_cast").
    Test hooks: `also` lists search outputs ("indices", "distances") declared as graph outputs too; `equal_values` replaces the branch
    constants 0 .. C - 1; `extra_reader` names an intermediate ("knn_all", "knn_lab" = the looked-up labels, "knn_wei") declared as one
    more graph output, which keeps the graph from being the pattern."""
    F, C = spec["features"], len(classes)
    nodes, inits, lab = _knn_vote_front(spec, y, k, weights, spelling, lookup, reshape, INT64 if cast else None, eps, reciprocal, np.int64)
    consts = list(range(C)) if equal_values is None else list(equal_values)
    inits.append(tensor("knn_axes1", np.array([1], np.int64)))
    if keepdims == 0:
        inits.append(tensor("knn_unsq", np.array([0 if join == "transpose" else 1], np.int64)))
    branches = []
    for c in range(C):
        inits.append(tensor(f"knn_c{c}", np.array(consts[c], np.int64)))
        nodes += [node("Equal", [lab, f"knn_c{c}"], [f"knn_eq{c}"], name=f"equal{c}"),
                  node("Cast", [f"knn_eq{c}"], [f"knn_f{c}"], [attr_i("to", FLOAT)], name=f"cast{c}")]
        cur = f"knn_f{c}"
        if weights == "distance":
            nodes.append(node("Mul", [cur, "knn_wei"], [f"knn_w{c}"], name=f"mul{c}"))
            cur = f"knn_w{c}"
        nodes.append(node("ReduceSum", [cur, "knn_axes1"], [f"knn_s{c}"], [attr_i("keepdims", keepdims)], name=f"sum{c}"))
        cur = f"knn_s{c}"
        if keepdims == 0:
            nodes.append(node("Unsqueeze", [cur, "knn_unsq"], [f"knn_u{c}"], name=f"unsqueeze{c}"))
            cur = f"knn_u{c}"
        branches.append(cur)
    if keepdims == 0 and join == "transpose":
        nodes += [node("Concat", branches, ["knn_all_t"], [attr_i("axis", 0)], name="concat"),
                  node("Transpose", ["knn_all_t"], ["knn_all"], [attr_ints("perm", [1, 0])], name="transpose")]
    else:
        nodes.append(node("Concat", branches, ["knn_all"], [attr_i("axis", 1)], name="concat"))
    nodes.append(node("ArgMax", ["knn_all"], ["knn_arg"], [attr_i("axis", 1), attr_i("keepdims", 0)], name="argmax"))
    inits.append(tensor("knn_classes", np.asarray(classes, np.int64)))
    if final is None:
        final = "reshape" if lookup == "afe" else "none"
    steps = {"none": [], "reshape": ["Reshape"], "cast": ["Cast"], "reshape_cast": ["Reshape", "Cast"]}[final]
    names = [f"knn_label{i}" for i in range(len(steps))] + ["label"]
    if lookup == "afe":
        nodes.append(node("ArrayFeatureExtractor", ["knn_classes", "knn_arg"], [names[0]], name="class_lookup", domain=ML_DOMAIN))
    else:
        nodes.append(node("Gather", ["knn_classes", "knn_arg"], [names[0]], [attr_i("axis", 0)], name="class_lookup"))
    for i, op in enumerate(steps):
        if op == "Reshape":
            inits.append(tensor("knn_label_shape", np.array([-1], np.int64)))
            nodes.append(node("Reshape", [names[i], "knn_label_shape"], [names[i + 1]], name="label_reshape"))
        else:
            nodes.append(node("Cast", [names[i]], [names[i + 1]], [attr_i("to", INT64)], name="label_cast"))
    nodes += [node("ReduceSum", ["knn_all", "knn_axes1"], ["knn_norm"], [attr_i("keepdims", 1)], name="norm"),
              node("Div", ["knn_all", "knn_norm"], ["probabilities"], name="proba")]
    proba = value_info("probabilities", ["N", C])
    if zipmap:
        nodes.append(node("ZipMap", ["probabilities"], ["output_probability"], [attr_ints("classlabels_int64s", [int(v) for v in classes])], name="zipmap", domain=ML_DOMAIN))
        proba = value_info("output_probability", ["N", C])
    outs = [value_info("label", ["N"], INT64), proba]
    if output == "probabilities":
        outs.reverse()
    elif output != "label":
        raise ValueError(output)
    for nm in also:
        outs.append(value_info(nm, ["N", k], INT64 if nm == "indices" else FLOAT))
    if extra_reader:
        nm = lab if extra_reader == "knn_lab" else extra_reader
        outs.append(value_info(nm, ["N", C] if nm == "knn_all" else ["N", k], INT64 if extra_reader == "knn_lab" else FLOAT))
    return _model_ms("knn_classifier", nodes, inits, [value_info("X", ["N", F])], outs) + _ld(8, _s(1, ML_DOMAIN) + _vi(2, 1))


def knn_regressor_from_spec(spec: dict, y, k: int = 5, weights: str = "uniform", spelling: str = "cdist", lookup: str = "afe", keepdims: int = 0,
                            reshape=None, eps: float = 1e-6, reciprocal: str = "reciprocal", final: str = "reshape") -> bytes:
    """KNeighborsRegressor as skl2onnx writes it, restated: `y` [M] are the training targets, float32 or an integer type (int64 in the graph,
    cast to FLOAT behind the lookup).  One output, `variable` [N, 1] (final = "none": the reduction's own shape).

    Recalled from the exporter's converter (convert_nearest_neighbors_regressor): the search head, the targets looked up by
    ArrayFeatureExtractor and reshaped to [-1, k], ReduceMean over axis 1 for uniform weights, ReduceSum(targets * weights) over ReduceSum(weights)
    for distance weights, a closing Reshape to [-1, 1].  Loose: `lookup`, `keepdims`, `reshape`, `reciprocal` as in knn_classifier_from_spec."""
    F = spec["features"]
    y = np.asarray(y)
    if final not in ("reshape", "none"):
        raise ValueError(final)
    integer = y.dtype.kind in "iu"  # (a 2-D y, the multi-output form [M, T], is written as it is: the lowering refuses it)
    nodes, inits, lab = _knn_vote_front(spec, y, k, weights, spelling, lookup, reshape, FLOAT if integer else None, eps, reciprocal, np.int64 if integer else np.float32)
    value = "variable" if final == "none" else "knn_value"
    if weights == "uniform":
        nodes.append(node("ReduceMean", [lab], [value], [attr_ints("axes", [1]), attr_i("keepdims", keepdims)], name="mean"))
    else:
        inits.append(tensor("knn_axes1", np.array([1], np.int64)))
        nodes += [node("Mul", [lab, "knn_wei"], ["knn_wt"], name="weighted"),
                  node("ReduceSum", ["knn_wt", "knn_axes1"], ["knn_num"], [attr_i("keepdims", keepdims)], name="num"),
                  node("ReduceSum", ["knn_wei", "knn_axes1"], ["knn_den"], [attr_i("keepdims", keepdims)], name="den"),
                  node("Div", ["knn_num", "knn_den"], [value], name="mean")]
    out = value_info("variable", ["N", 1] if final == "reshape" or keepdims else ["N"])
    if final == "reshape":
        inits.append(tensor("knn_out_shape", np.array([-1, 1], np.int64)))
        nodes.append(node("Reshape", ["knn_value", "knn_out_shape"], ["variable"], name="out_reshape"))
    return _model_ms("knn_regressor", nodes, inits, [value_info("X", ["N", F])], [out]) + _ld(8, _s(1, ML_DOMAIN) + _vi(2, 1))


def nearest_reference(spec: dict, x, k: int = 1) -> dict:
    """float64 restatement: d2 [N, M] (NaN rows stay NaN), label, the k nearest `indices` (stable: equal distances by lower index, NaN after
    every number) and `values` (d2), `gap_out` = d2 of the (k+1)-th minus the k-th (inf when k = M), `gap_in` = the smallest gap between
    neighbours inside the top k (inf when k = 1), and `mag` [N, M] = |xc|^2 + |cc|^2 + 2 sum |xc_f cc_f| with xc = x - mu, cc = c - mu
    (mu = the mean of the set): the magnitude the error of the centred evaluation scales with."""
    C = np.asarray(spec["centers"], dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    mu = C.mean(0).astype(np.float32).astype(np.float64)
    xc, cc = x - mu, C - mu
    M = C.shape[0]
    d2 = np.empty((x.shape[0], M))
    mag = np.empty((x.shape[0], M))
    for r0 in range(0, x.shape[0], 256):
        diff = x[r0:r0 + 256, None, :] - C[None, :, :]
        d2[r0:r0 + 256] = (diff * diff).sum(-1)
        mag[r0:r0 + 256] = (xc[r0:r0 + 256] ** 2).sum(1)[:, None] + (cc ** 2).sum(1)[None, :] + 2 * np.abs(xc[r0:r0 + 256, None, :] * cc[None, :, :]).sum(-1)
    key = np.where(np.isnan(d2), np.inf, d2)
    order = np.argsort(key, axis=1, kind="stable")
    srt = np.take_along_axis(d2, order, 1)
    ksrt = np.take_along_axis(key, order, 1)
    with np.errstate(invalid="ignore"):  # (a NaN row: inf - inf)
        gap_out = ksrt[:, k] - ksrt[:, k - 1] if k < M else np.full(x.shape[0], np.inf)
        gap_in = np.diff(ksrt[:, :k], axis=1).min(1) if k > 1 else np.full(x.shape[0], np.inf)
    return {"d2": d2, "label": order[:, 0], "indices": order[:, :k], "values": srt[:, :k], "gap_out": gap_out, "gap_in": gap_in, "mag": mag}


def reduce_zoo(rank: int = 2, F: int = 5, T: int = 3, keepdims: int = 1, k: int = 3, axes_input: bool = False, opset: int = 13) -> tuple[bytes, list]:
    """One graph output per reduction operator over the last axis of X ([N, F], or for rank 3 the window [N, T, F] of a flat [N, T * F] input), then -- rank 2 only --
    ArgMin, TopK (both directions, values and indices) and the row-scalar broadcast in every operand order.  Returns (model, output names).
    axes_input: `axes` as a constant input (the opset-18 form) instead of the attribute."""
    dims = ["N", F] if rank == 2 else ["N", T, F]
    red = dims[:-1] + ([1] if keepdims else [])
    nodes, inits, outs = [], [], []
    if rank == 3:  # the window arrives flat, [N, T * F] (what the C ABI and the SQL surface carry), and is reshaped in the graph
        inits.append(tensor("win_shape", np.array([0, T, F], np.int64)))
        nodes.append(node("Reshape", ["X_flat", "win_shape"], ["X"], name="window"))
    if axes_input:
        inits.append(tensor("axes", np.array([-1], np.int64)))
    for op in REDUCE_OPS:
        o = "r_" + op
        if axes_input:
            nodes.append(node(op, ["X", "axes"], [o], [attr_i("keepdims", keepdims)], name=op))
        else:
            nodes.append(node(op, ["X"], [o], [attr_ints("axes", [rank - 1]), attr_i("keepdims", keepdims)], name=op))
        outs.append(value_info(o, red))
    names = ["r_" + op for op in REDUCE_OPS]
    # the row-scalar broadcast reads a keepdims = 1 reduction of its own
    nodes.append(node("ReduceMax", ["X"], ["b_s"], [attr_ints("axes", [rank - 1]), attr_i("keepdims", 1)], name="b_scalar"))
    for op in ("Add", "Sub", "Mul", "Div", "Min", "Max"):
        for side, ins in (("r", ["X", "b_s"]), ("l", ["b_s", "X"])):
            o = f"b_{op}_{side}"
            nodes.append(node(op, ins, [o], name=o))
            outs.append(value_info(o, dims))
            names.append(o)
    if rank == 2:
        inits.append(tensor("topk_k", np.array([k], np.int64)))
        nodes.append(node("ArgMin", ["X"], ["argmin"], [attr_i("axis", 1), attr_i("keepdims", 0)], name="argmin"))
        outs.append(value_info("argmin", ["N"], INT64))
        names.append("argmin")
        for largest in (0, 1):
            v, i = f"topk_v{largest}", f"topk_i{largest}"
            nodes.append(node("TopK", ["X", "topk_k"], [v, i], [attr_i("axis", -1), attr_i("largest", largest)], name=f"topk{largest}"))
            outs += [value_info(v, ["N", k]), value_info(i, ["N", k], INT64)]
            names += [v, i]
    x_in = value_info("X", dims) if rank == 2 else value_info("X_flat", ["N", T * F])
    return model("reduce_zoo", nodes, inits, [x_in], outs, opset=opset), names


def reduce_reference(x, k: int = 3) -> dict:
    """float64 numpy values of every reduce_zoo() output (keepdims = 1 shapes; squeeze for keepdims = 0), with `mag_<op>` = the sum of
    absolute terms the rounding error of the summed operators scales with."""
    x = np.asarray(x, dtype=np.float64)
    kd = dict(axis=-1, keepdims=True)
    mx = x.max(**kd)
    with np.errstate(all="ignore"):
        out = {"r_ReduceSum": x.sum(**kd), "r_ReduceMean": x.mean(**kd), "r_ReduceMax": mx, "r_ReduceMin": x.min(**kd), "r_ReduceProd": x.prod(**kd),
               "r_ReduceL1": np.abs(x).sum(**kd), "r_ReduceL2": np.sqrt((x * x).sum(**kd)), "r_ReduceSumSquare": (x * x).sum(**kd),
               "r_ReduceLogSum": np.log(x.sum(**kd)), "r_ReduceLogSumExp": np.log(np.exp(x - mx).sum(**kd)) + mx}
        s = mx
        for op, f in (("Add", np.add), ("Sub", np.subtract), ("Mul", np.multiply), ("Div", np.divide), ("Min", np.minimum), ("Max", np.maximum)):
            out[f"b_{op}_r"], out[f"b_{op}_l"] = f(x, s), f(s, x)
    out["mag_sum"] = np.abs(x).sum(**kd)
    if x.ndim == 2:
        out["argmin"] = np.argmin(x, 1)
        for largest in (0, 1):
            order = np.argsort(-x if largest else x, axis=1, kind="stable")[:, :k]
            out[f"topk_i{largest}"], out[f"topk_v{largest}"] = order, np.take_along_axis(x, order, 1)
    return out


def autoencoder(F: int = 12, H: int = 4, seed: int = 31) -> tuple[bytes, dict]:
    """Reconstruction error mean((x - dec(enc(x)))^2, axis 1): Gemm(Relu) -> Gemm -> Sub -> Mul -> ReduceMean.  Returns (model, weights)."""
    ws = _WeightStream(seed)
    w = {"W1": ws.take((F, H), F), "b1": ws.take((H,), F), "W2": ws.take((H, F), H), "b2": ws.take((F,), H)}
    nodes = [node("Gemm", ["X", "W1", "b1"], ["h0"], name="enc"), node("Relu", ["h0"], ["h"], name="relu"), node("Gemm", ["h", "W2", "b2"], ["rec"], name="dec"),
             node("Sub", ["X", "rec"], ["diff"], name="sub"), node("Mul", ["diff", "diff"], ["sq"], name="mul"),
             node("ReduceMean", ["sq"], ["err"], [attr_ints("axes", [1]), attr_i("keepdims", 0)], name="mean")]
    return model("autoencoder", nodes, [tensor(k, v) for k, v in w.items()], [value_info("X", ["N", F])], [value_info("err", ["N"])], opset=13), w


# ------------------------------------------------------------------------------------------
# decoders: ConvTranspose, Resize and Upsample with their float64 references.  The references are written
# from the operator specification's definitions: they play the oracle's part for these operators.
# ------------------------------------------------------------------------------------------

def _pair(v) -> tuple:
    return (int(v), int(v)) if np.isscalar(v) else tuple(int(t) for t in v)


def _pads4(p) -> tuple:
    if np.isscalar(p):
        return (int(p),) * 4
    p = tuple(int(t) for t in p)
    return p if len(p) == 4 else (p[0], p[1], p[0], p[1])


def conv_transpose_pads(in_hw, k, strides, dilations, output_padding, output_shape=None, auto_pad: str = "NOTSET", pads=(0, 0, 0, 0)) -> tuple:
    """(pt, pl, pb, pr) of a ConvTranspose as the specification derives them from output_shape / auto_pad."""
    if auto_pad == "VALID":
        return (0, 0, 0, 0)
    if output_shape is None and auto_pad == "NOTSET":
        return _pads4(pads)
    begin, end = [], []
    for ax in range(2):
        want = output_shape[ax] if output_shape is not None else in_hw[ax] * strides[ax]
        total = strides[ax] * (in_hw[ax] - 1) + output_padding[ax] + (k[ax] - 1) * dilations[ax] + 1 - want
        b = total // 2 if auto_pad == "SAME_UPPER" else total - total // 2
        begin.append(b)
        end.append(total - b)
    return (begin[0], begin[1], end[0], end[1])


def conv_transpose_reference(x, w, b=None, strides=1, pads=0, dilations=1, groups: int = 1, output_padding=0) -> np.ndarray:
    """ONNX ConvTranspose in float64, from its definition: every input pixel (ih, iw) adds x * w[:, :, ky, kx] at output position
    (ih * sh + ky * dh - pt, iw * sw + kx * dw - pl).  x [N,C,H,W] with w [C,M/g,kh,kw], or x [N,C,L] with w [C,M/g,k]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    if x.ndim == 3:
        one = lambda v: v if np.isscalar(v) else v[0]
        p = (pads, pads) if np.isscalar(pads) else tuple(pads)
        y = conv_transpose_reference(x[:, :, None, :], w[:, :, None, :], b, (1, one(strides)), (0, p[0], 0, p[1]), (1, one(dilations)), groups,
                                     (0, one(output_padding)))
        return y[:, :, 0, :]
    (sh, sw), (pt, pl, pb, pr), (dh, dw), (oph, opw) = _pair(strides), _pads4(pads), _pair(dilations), _pair(output_padding)
    n, c, h, wd = x.shape
    _, mg, kh, kw = w.shape
    cg = c // groups
    fh, fw = (h - 1) * sh + dh * (kh - 1) + 1 + oph, (wd - 1) * sw + dw * (kw - 1) + 1 + opw
    full = np.zeros((n, mg * groups, fh, fw), np.float64)
    for g in range(groups):
        for ky in range(kh):
            for kx in range(kw):
                full[:, g * mg:(g + 1) * mg, ky * dh:ky * dh + (h - 1) * sh + 1:sh, kx * dw:kx * dw + (wd - 1) * sw + 1:sw] += np.einsum(
                    "nchw,cm->nmhw", x[:, g * cg:(g + 1) * cg], w[g * cg:(g + 1) * cg, :, ky, kx], optimize=True)
    out = full[:, :, pt:fh - pb, pl:fw - pr]
    if b is not None:
        out = out + np.asarray(b, np.float64)[None, :, None, None]
    return out


def resize_axis_reference(n_in: int, n_out: int, scale: float, mode: str, coord: str, nearest_mode: str = "round_prefer_floor"):
    """One axis of Resize: nearest -> the source index per output coordinate; linear -> (i0, i1, w).  float64, the specification's formulas."""
    o = np.arange(n_out, dtype=np.float64)
    if coord == "half_pixel":
        x = (o + 0.5) / scale - 0.5
    elif coord == "pytorch_half_pixel":
        x = (o + 0.5) / scale - 0.5 if n_out > 1 else np.zeros_like(o)
    elif coord == "align_corners":
        x = o * (n_in - 1) / (n_out - 1) if n_out > 1 else np.zeros_like(o)
    elif coord == "asymmetric":
        x = o / scale
    else:
        raise ValueError(coord)
    if mode == "nearest":
        r = {"round_prefer_floor": np.ceil(x - 0.5), "round_prefer_ceil": np.floor(x + 0.5), "floor": np.floor(x), "ceil": np.ceil(x)}[nearest_mode]
        return np.clip(r, 0, n_in - 1).astype(np.int64)
    x = np.clip(x, 0, n_in - 1)
    i0 = np.floor(x).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), x - i0


def resize_reference(x, sizes=None, scales=None, mode: str = "nearest", coord: str = "half_pixel", nearest_mode: str = "round_prefer_floor") -> np.ndarray:
    """ONNX Resize (nearest / linear) of x [N,C,H,W] or [N,C,L] in float64; `sizes` / `scales` cover the spatial axes only."""
    x = np.asarray(x, np.float64)
    if x.ndim == 3:
        one = lambda v: None if v is None else (1, v if np.isscalar(v) else v[-1])
        return resize_reference(x[:, :, None, :], one(sizes), one(scales), mode, coord, nearest_mode)[:, :, 0, :]
    out = x
    for ax in (2, 3):
        n_in = x.shape[ax]
        if scales is not None:
            sc = float(_pair_f(scales)[ax - 2])
            n_out = int(math.floor(n_in * sc))
        else:
            n_out = int(_pair(sizes)[ax - 2])
            sc = n_out / n_in
        t = resize_axis_reference(n_in, n_out, sc, mode, coord, nearest_mode)
        if mode == "nearest":
            out = np.take(out, t, axis=ax)
        else:
            i0, i1, w = t
            shape = [1, 1, 1, 1]
            shape[ax] = n_out
            w = w.reshape(shape)
            out = (1.0 - w) * np.take(out, i0, axis=ax) + w * np.take(out, i1, axis=ax)
    return out


def _pair_f(v) -> tuple:
    return (float(v), float(v)) if np.isscalar(v) else tuple(float(t) for t in v)


class _DecoderNet:
    """Records a small convolutional graph twice: as ONNX nodes and as layer descriptors decoder_reference() evaluates in float64."""

    def __init__(self, seed: int, integer: bool = False):
        self.rng = np.random.default_rng(seed)
        self.integer = integer
        self.nodes, self.inits, self.layers, self.count = [], [], [], 0

    def draw(self, shape, fan):
        if self.integer:
            return self.rng.integers(-8, 9, size=shape).astype(np.float32)
        return (self.rng.uniform(-1, 1, size=shape) / math.sqrt(max(fan, 1))).astype(np.float32)

    def _name(self, op):
        self.count += 1
        return f"{op}{self.count}"

    def const(self, name, arr):
        self.inits.append(tensor(name, arr))
        return name

    def conv(self, x, c, m, k=3, s=1, p=0, groups=1, bias=True, w=None, one_d=False):
        nm = self._name("conv")
        k2, s2, p4 = _pair(k), _pair(s), _pads4(p)
        if one_d:
            k2, s2, p4 = (1, k2[1]), (1, s2[1]), (0, p4[1], 0, p4[3])
        w = self.draw((m, c // groups) + k2, (c // groups) * k2[0] * k2[1]) if w is None else w
        b = self.draw((m,), (c // groups) * k2[0] * k2[1]) if bias else None
        ins = [x, self.const(nm + "_W", w[:, :, 0, :] if one_d else w)] + ([self.const(nm + "_B", b)] if bias else [])
        attrs = ([attr_ints("kernel_shape", [k2[1]]), attr_ints("strides", [s2[1]]), attr_ints("pads", [p4[1], p4[3]])] if one_d else
                 [attr_ints("kernel_shape", k2), attr_ints("strides", s2), attr_ints("pads", p4)]) + [attr_i("group", groups)]
        self.nodes.append(node("Conv", ins, [nm], attrs, name=nm))
        self.layers.append(("conv", nm, [x], dict(w=w, b=b, strides=s2, pads=p4, groups=groups)))
        return nm

    def convt(self, x, c, m, k=2, s=2, p=0, d=1, groups=1, op=0, bias=True, w=None, one_d=False, output_shape=None, auto_pad="NOTSET", in_hw=None,
              name=None):
        nm = name or self._name("convt")
        k2, s2, d2, op2 = _pair(k), _pair(s), _pair(d), _pair(op)
        if one_d:
            k2, s2, d2, op2 = (1, k2[1]), (1, s2[1]), (1, d2[1]), (0, op2[1])
        w = self.draw((c, m // groups) + k2, (c // groups) * k2[0] * k2[1]) if w is None else w
        b = self.draw((m,), (c // groups) * k2[0] * k2[1]) if bias else None
        ins = [x, self.const(nm + "_W", w[:, :, 0, :] if one_d else w)] + ([self.const(nm + "_B", b)] if bias else [])
        sel = (lambda v: [v[1]]) if one_d else (lambda v: list(v))
        attrs = [attr_ints("strides", sel(s2)), attr_ints("dilations", sel(d2)), attr_i("group", groups)]
        if any(op2):
            attrs.append(attr_ints("output_padding", sel(op2)))
        if output_shape is not None or auto_pad != "NOTSET":
            if output_shape is not None:
                attrs.append(attr_ints("output_shape", list(output_shape)))
            if auto_pad != "NOTSET":
                attrs.append(attr_s("auto_pad", auto_pad))
            p4 = conv_transpose_pads(in_hw, k2, s2, d2, op2, output_shape, auto_pad)
        else:
            p4 = _pads4(p)
            if one_d:
                p4 = (0, p4[1], 0, p4[3])
            attrs.append(attr_ints("pads", [p4[1], p4[3]] if one_d else p4))
        self.nodes.append(node("ConvTranspose", ins, [nm], attrs, name=nm))
        self.layers.append(("convt", nm, [x], dict(w=w, b=b, strides=s2, pads=p4, dilations=d2, groups=groups, output_padding=op2)))
        return nm

    def bn(self, x, c):
        nm = self._name("bn")
        sc, bi, mu = (self.rng.uniform(0.5, 1.5, c).astype(np.float32), self.rng.uniform(-0.5, 0.5, c).astype(np.float32),
                      self.rng.uniform(-0.5, 0.5, c).astype(np.float32))
        var = self.rng.uniform(0.5, 2.0, c).astype(np.float32)
        ins = [x] + [self.const(f"{nm}_{k}", v) for k, v in (("scale", sc), ("bias", bi), ("mean", mu), ("var", var))]
        self.nodes.append(node("BatchNormalization", ins, [nm], [attr_f("epsilon", 1e-5)], name=nm))
        self.layers.append(("bn", nm, [x], dict(scale=sc, bias=bi, mean=mu, var=var, eps=float(np.float32(1e-5)))))
        return nm

    def act(self, x, op="Relu"):
        nm = self._name(op.lower())
        self.nodes.append(node(op, [x], [nm], name=nm))
        self.layers.append((op.lower(), nm, [x], {}))
        return nm

    def concat(self, xs):
        nm = self._name("concat")
        self.nodes.append(node("Concat", list(xs), [nm], [attr_i("axis", 1)], name=nm))
        self.layers.append(("concat", nm, list(xs), {}))
        return nm

    def resize(self, x, rank=4, scales=None, sizes=None, mode="nearest", coord="asymmetric", nearest_mode="floor", op="Resize", opset=13, attrs_extra=(),
               lead=None):
        nm = self._name("resize")
        lead_s = [1.0, 1.0]
        if scales is not None:
            sp = list(_pair_f(scales))[-(rank - 2):]  # (the spatial axes: the last one alone for [N,C,L])
            sc = self.const(nm + "_scales", np.asarray(lead_s + sp, np.float32) if lead is None else np.asarray(list(lead) + sp, np.float32))
        if op == "Upsample":
            attrs = [attr_s("mode", mode)]
            if opset < 9:
                attrs.append(attr_floats("scales", lead_s + sp))
                ins = [x]
            else:
                ins = [x, sc]
        elif opset < 11:
            attrs, ins = [attr_s("mode", mode)], [x, sc]
        else:
            attrs = [attr_s("mode", mode), attr_s("coordinate_transformation_mode", coord), attr_s("nearest_mode", nearest_mode)]
            if scales is not None:
                ins = [x, "", sc]
            else:
                ins = [x, "", "", self.const(nm + "_sizes", np.asarray(list(lead if lead is not None else (0, sizes[0])) + list(sizes[1:]), np.int64))]
        self.nodes.append(node(op, ins, [nm], list(attrs) + list(attrs_extra), name=nm))
        old = op == "Upsample" or opset < 11
        self.layers.append(("resize", nm, [x], dict(scales=None if scales is None else sp, sizes=None if sizes is None else list(sizes[1:]), mode=mode,
                                                    coord="asymmetric" if old else coord, nearest_mode="floor" if old else nearest_mode)))
        return nm

    def silu(self, x):
        """x * Sigmoid(x), as exporters spell SiLU / Swish"""
        nm = self._name("silu")
        self.nodes.append(node("Sigmoid", [x], [nm + "_sig"], name=nm + "_sig"))
        self.nodes.append(node("Mul", [x, nm + "_sig"], [nm], name=nm))
        self.layers.append(("silu", nm, [x], {}))
        return nm

    def add(self, a, b):
        nm = self._name("add")
        self.nodes.append(node("Add", [a, b], [nm], name=nm))
        self.layers.append(("add", nm, [a, b], {}))
        return nm

    def _norm_params(self, n):
        return self.rng.uniform(0.5, 1.5, n).astype(np.float32), self.rng.uniform(-0.5, 0.5, n).astype(np.float32)

    def inorm(self, x, c, eps=1e-5, name=None):
        """InstanceNormalization with per-channel scale and B"""
        nm = name or self._name("inorm")
        g, b = self._norm_params(c)
        self.nodes.append(node("InstanceNormalization", [x, self.const(nm + "_scale", g), self.const(nm + "_B", b)], [nm], [attr_f("epsilon", eps)], name=nm))
        self.layers.append(("inorm", nm, [x], dict(groups=c, gamma=g, beta=b, eps=float(np.float32(eps)))))
        return nm

    def gnorm(self, x, c, groups, form="op21", inner=None, eps=1e-5, name=None, back="const", affine="mul_add", x_shape=None):
        """GroupNormalization.  form "op18": scale / bias per group (opset 18); "op21": per channel (opset 21); "exporter": what torch.onnx
        writes for nn.GroupNorm below opset 18 -- Reshape [0, G, -1], InstanceNormalization with `inner` = (scale[G], B[G]) (None: ones and
        zeros), Reshape back (`back`: a constant shape, or "shape": Shape(x); x_shape = x's extents behind the row axis), then Mul(gamma
        [C,1,1]) and Add(beta) (`affine`: "mul_add", "mul", "none").  The layer records the per-channel gamma and beta of the whole spelling
        in float64."""
        nm = name or self._name("gnorm")
        e32 = float(np.float32(eps))
        if form in ("op18", "op21"):
            g, b = self._norm_params(groups if form == "op18" else c)
            self.nodes.append(node("GroupNormalization", [x, self.const(nm + "_scale", g), self.const(nm + "_bias", b)], [nm],
                                   [attr_i("num_groups", groups), attr_f("epsilon", eps)], name=nm))
            rep = c // groups if form == "op18" else 1
            self.layers.append(("gnorm", nm, [x], dict(groups=groups, gamma=np.repeat(g, rep), beta=np.repeat(b, rep), eps=e32)))
            return nm
        if form != "exporter":
            raise ValueError(form)
        s, b = (np.ones(groups, np.float32), np.zeros(groups, np.float32)) if inner is None else (np.asarray(inner[0], np.float32), np.asarray(inner[1], np.float32))
        gamma, beta = self._norm_params(c)
        one = (1,) * len(x_shape[1:])
        self.nodes.append(node("Reshape", [x, self.const(nm + "_to_groups", np.asarray([0, groups, -1], np.int64))], [nm + "_g"], name=nm + "_split"))
        self.nodes.append(node("InstanceNormalization", [nm + "_g", self.const(nm + "_scale", s), self.const(nm + "_B", b)], [nm + "_n"], [attr_f("epsilon", eps)], name=nm + "_inorm"))
        if back == "shape":
            self.nodes.append(node("Shape", [x], [nm + "_shape"], name=nm + "_shape"))
            shape_in = nm + "_shape"
        else:
            shape_in = self.const(nm + "_back", np.asarray([0] + list(x_shape), np.int64))
        cur = nm if affine == "none" else nm + "_r"
        self.nodes.append(node("Reshape", [nm + "_n", shape_in], [cur], name=nm + "_merge"))
        if affine in ("mul", "mul_add"):
            nxt = nm if affine == "mul" else nm + "_m"
            self.nodes.append(node("Mul", [cur, self.const(nm + "_gamma", gamma.reshape((c,) + one))], [nxt], name=nm + "_mul"))
            cur = nxt
        if affine == "mul_add":
            self.nodes.append(node("Add", [cur, self.const(nm + "_beta", beta.reshape((1, c) + one))], [nm], name=nm + "_add"))
        g64 = gamma.astype(np.float64) if affine != "none" else np.ones(c)
        b64 = beta.astype(np.float64) if affine == "mul_add" else np.zeros(c)
        rep = c // groups
        self.layers.append(("gnorm", nm, [x], dict(groups=groups, gamma=np.repeat(s.astype(np.float64), rep) * g64, beta=np.repeat(b.astype(np.float64), rep) * g64 + b64, eps=e32)))
        return nm

    def shuffle(self, x, c, hw, form="crd", b=2, spelling=False, mode_attr=True, lead=0, target="const", perm=None, name=None, attrs_extra=()):
        """One sub-pixel layer over x [N, c, *hw].  form: "dcr" / "crd" (DepthToSpace), "s2d" (SpaceToDepth), "unshuffle" (F.pixel_unshuffle:
        a spelling only).  spelling: Reshape -> Transpose -> Reshape (nodes <name>_split, <name>_perm, <name>_merge) in place of the operator;
        b: the block size, or (b_h, b_w) in a spelling; lead: the targets' row entry (0 or -1); target = "shape": the first target's row entry
        is cut from Shape(x); perm: another permutation than the form's.  mode_attr = False: DepthToSpace without its mode (DCR).
        Returns (result, its (C, H, W))."""
        nm = name or self._name("shuffle")
        bh, bw = _pair(b)
        h, w = hw
        to_space = form in ("dcr", "crd")
        oshape = (c // (bh * bw), h * bh, w * bw) if to_space else (c * bh * bw, h // bh, w // bw)
        if not spelling:
            if form == "unshuffle":
                raise ValueError("pixel_unshuffle has no operator")
            attrs = [attr_i("blocksize", bh)] + ([attr_s("mode", form.upper())] if to_space and (mode_attr or form == "crd") else [])
            self.nodes.append(node("DepthToSpace" if to_space else "SpaceToDepth", [x], [nm], attrs + list(attrs_extra), name=nm))
        else:
            six, pm = PIXEL_SHUFFLE_SPELLINGS[form]
            dims = dict(N=lead, b1=bh, b2=bw, Cs=oshape[0], C=c, H=h, W=w, Hb=h // bh, Wb=w // bw)
            t1 = [dims[k] for k in six]
            if target == "shape":
                self.nodes.append(node("Shape", [x], [nm + "_shape"], name=nm + "_shape"))
                self.nodes.append(node("Gather", [nm + "_shape", self.const(nm + "_zero", np.asarray([0], np.int64))], [nm + "_n"], [attr_i("axis", 0)], name=nm + "_n"))
                self.nodes.append(node("Concat", [nm + "_n", self.const(nm + "_rest", np.asarray(t1[1:], np.int64))], [nm + "_t1"], [attr_i("axis", 0)], name=nm + "_t1"))
                t1_in = nm + "_t1"
            else:
                t1_in = self.const(nm + "_t1", np.asarray(t1, np.int64))
            self.nodes.append(node("Reshape", [x, t1_in], [nm + "_6d"], name=nm + "_split"))
            self.nodes.append(node("Transpose", [nm + "_6d"], [nm + "_t"], [attr_ints("perm", perm or pm)], name=nm + "_perm"))
            self.nodes.append(node("Reshape", [nm + "_t", self.const(nm + "_t2", np.asarray([lead] + list(oshape), np.int64))], [nm], name=nm + "_merge"))
        self.layers.append(("shuffle", nm, [x], dict(form=form, b=(bh, bw))))
        return nm, oshape

    def finish(self, name, x_info, out, out_dims, opset=13, extra=None):
        spec = {"layers": self.layers, "output": out}
        spec.update(extra or {})
        return model(name, self.nodes, self.inits, [x_info], [value_info(out, out_dims)], opset=opset), spec


def decoder_reference(spec: dict, x, upto: str | None = None) -> np.ndarray:
    """The graph a _DecoderNet recorded, in float64 (BatchNormalization as the operator defines it, unfolded)."""
    vals = {"X": np.asarray(x, np.float64).reshape((len(x),) + tuple(spec["in_shape"]))}
    for op, out, ins, p in spec["layers"]:
        a = vals[ins[0]]
        if op == "conv":
            squeeze = a.ndim == 3
            a4 = a[:, :, None, :] if squeeze else a
            y = _conv_taps(a4, p["w"].astype(np.float64), p["strides"], p["pads"], (1, 1), p["groups"], 0.0)
            if p["b"] is not None:
                y = y + p["b"].astype(np.float64)[None, :, None, None]
            y = y[:, :, 0, :] if squeeze else y
        elif op == "convt":
            squeeze = a.ndim == 3
            a4 = a[:, :, None, :] if squeeze else a
            y = conv_transpose_reference(a4, p["w"], p["b"], p["strides"], p["pads"], p["dilations"], p["groups"], p["output_padding"])
            y = y[:, :, 0, :] if squeeze else y
        elif op == "bn":
            sh = (1, -1) + (1,) * (a.ndim - 2)
            f = lambda k: p[k].astype(np.float64).reshape(sh)
            y = (a - f("mean")) / np.sqrt(f("var") + p["eps"]) * f("scale") + f("bias")
        elif op == "relu":
            y = np.maximum(a, 0.0)
        elif op == "sigmoid":
            y = 1.0 / (1.0 + np.exp(-a))
        elif op == "tanh":
            y = np.tanh(a)
        elif op == "softplus":
            y = np.log1p(np.exp(a))
        elif op == "concat":
            y = np.concatenate([vals[i] for i in ins], axis=1)
        elif op == "resize":
            y = resize_reference(a, sizes=p["sizes"], scales=p["scales"], mode=p["mode"], coord=p["coord"], nearest_mode=p["nearest_mode"])
        elif op == "reshape":
            y = a.reshape((len(a),) + tuple(p["shape"]))
        elif op == "shuffle":
            y = pixel_shuffle_apply(a, p["form"], p["b"])
        elif op in ("inorm", "gnorm"):
            y = spatialnorm_reference(a, p["groups"], p["gamma"], p["beta"], p["eps"])
        elif op == "silu":
            y = a / (1.0 + np.exp(-a))
        elif op == "add":
            y = a + vals[ins[1]]
        elif op == "sub":
            y = a - vals[ins[1]]
        elif op == "gap":
            y = a.mean(axis=(2, 3), keepdims=True)
        elif op == "sumsquare":
            y = (a * a).sum(axis=1)
        else:
            raise ValueError(op)
        vals[out] = y
        if out == upto:
            break
    return vals[upto or spec["output"]]


def conv_transpose_model(geom: dict, pre: bool = False, post: bool = False, act: str | None = None, bn: bool = False, integer: bool = False,
                         bias: bool = True, seed: int = 5, name: str = "convt") -> tuple[bytes, dict]:
    """One ConvTranspose layer `name`.  geom: C, M, H, W (H absent: 1-D, input [N,C,W]), k, s, p (pads), d, g, op (output_padding), output_shape,
    auto_pad.  pre: an identity 1x1 Conv in front (the layer then reads a channel-quad tensor where C is whole quads); post: an identity
    1x1 ConvTranspose behind it (the layer then writes one).  integer: weights and bias are whole numbers in [-8, 8].  Returns (model, spec)."""
    one_d = "H" not in geom
    c, m, h, wd = geom["C"], geom["M"], geom.get("H", 1), geom["W"]
    net = _DecoderNet(seed, integer)
    cur = "X"
    if pre:
        eye = np.eye(c, dtype=np.float32)[:, :, None, None]
        cur = net.conv(cur, c, c, 1, 1, 0, bias=False, w=eye, one_d=one_d)
    cur = net.convt(cur, c, m, geom.get("k", 2), geom.get("s", 2), geom.get("p", 0), geom.get("d", 1), geom.get("g", 1), geom.get("op", 0), bias=bias,
                    one_d=one_d, output_shape=geom.get("output_shape"), auto_pad=geom.get("auto_pad", "NOTSET"), in_hw=(h, wd), name=name)
    if bn:
        cur = net.bn(cur, m)
    if act:
        cur = net.act(cur, act)
    if post:
        eye = np.eye(m, dtype=np.float32)[:, :, None, None]
        cur = net.convt(cur, m, m, 1, 1, 0, bias=False, w=eye, one_d=one_d)
    in_shape = (c, wd) if one_d else (c, h, wd)
    out_shape = decoder_reference({"layers": net.layers, "output": cur, "in_shape": in_shape}, np.zeros((1,) + in_shape)).shape[1:]
    return net.finish("conv_transpose", value_info("X", ["N"] + list(in_shape)), cur, ["N"] + list(out_shape), extra={"in_shape": in_shape, "out_shape": out_shape})


def resize_model(c: int = 3, hw=(4, 4), scales=None, sizes=None, mode: str = "nearest", coord: str = "half_pixel", nearest_mode: str = "round_prefer_floor",
                 op: str = "Resize", opset: int = 13, pre: bool = False, post: bool = False, attrs_extra=(), lead=None) -> tuple[bytes, dict]:
    """One Resize (or Upsample) node.  hw: (H, W), or (L,) for an [N,C,L] input; sizes: the output's (H, W) / (L,).  pre / post: identity 1x1 layers
    around it as in conv_transpose_model (the node then runs on channel-quad tensors).  lead: the N and C entries of scales / sizes."""
    one_d = len(hw) == 1
    net = _DecoderNet(0)
    cur = "X"
    if pre:
        cur = net.conv(cur, c, c, 1, 1, 0, bias=False, w=np.eye(c, dtype=np.float32)[:, :, None, None], one_d=one_d)
    rank = 3 if one_d else 4
    cur = net.resize(cur, rank, scales=scales, sizes=None if sizes is None else [c] + list(sizes), mode=mode, coord=coord, nearest_mode=nearest_mode, op=op, opset=opset,
                     attrs_extra=attrs_extra, lead=lead)
    if post:
        cur = net.convt(cur, c, c, 1, 1, 0, bias=False, w=np.eye(c, dtype=np.float32)[:, :, None, None], one_d=one_d)
    in_shape = (c,) + tuple(hw)
    out_shape = decoder_reference({"layers": net.layers, "output": cur, "in_shape": in_shape}, np.zeros((1,) + in_shape)).shape[1:]
    return net.finish("resize", value_info("X", ["N"] + list(in_shape)), cur, ["N"] + list(out_shape), opset=opset, extra={"in_shape": in_shape, "out_shape": out_shape})


def conv_autoencoder(channels: Sequence[int] = (3, 16, 32), size: int = 16, seed: int = 41) -> tuple[bytes, dict]:
    """Image autoencoder: stride-2 Conv 3x3 + Relu per level down, ConvTranspose k4 s2 p1 + BatchNormalization + Relu per level up, the last
    level ConvTranspose + Sigmoid.  Returns (model, spec) for decoder_reference."""
    net = _DecoderNet(seed)
    cur = "X"
    for a, b in zip(channels[:-1], channels[1:]):
        cur = net.act(net.conv(cur, a, b, 3, 2, 1), "Relu")
    rev = list(channels[::-1])
    for i, (a, b) in enumerate(zip(rev[:-1], rev[1:])):
        cur = net.convt(cur, a, b, 4, 2, 1)
        cur = net.act(cur, "Sigmoid") if i == len(rev) - 2 else net.act(net.bn(cur, b), "Relu")
    shape = (channels[0], size, size)
    return net.finish("conv_autoencoder", value_info("X", ["N"] + list(shape)), cur, ["N"] + list(shape), extra={"in_shape": shape})


def conv1d_autoencoder(T: int = 16, F: int = 4, hidden: Sequence[int] = (8, 16), seed: int = 43) -> tuple[bytes, dict]:
    """Anomaly score of a window of sensor readings served from a flat table: the T * F columns (feature-major: column f * T + t) are reshaped
    to [N, F, T] inside the model, encoded by stride-2 Conv1d + Relu, decoded by ConvTranspose1d k4 s2 p1, and the output is the
    reconstruction error sum((x - rec)^2) per row (ReduceSumSquare)."""
    net = _DecoderNet(seed)
    net.const("shape_ft", np.asarray([0, F, T], np.int64))
    net.nodes.append(node("Reshape", ["X", "shape_ft"], ["x3"], name="to_window"))
    net.layers.append(("reshape", "x3", ["X"], dict(shape=(F, T))))
    cur, chans = "x3", [F] + list(hidden)
    for a, b in zip(chans[:-1], chans[1:]):
        cur = net.act(net.conv(cur, a, b, 3, 2, 1, one_d=True), "Relu")
    rev = chans[::-1]
    for i, (a, b) in enumerate(zip(rev[:-1], rev[1:])):
        cur = net.convt(cur, a, b, 4, 2, 1, one_d=True)
        if i < len(rev) - 2:
            cur = net.act(cur, "Relu")
    net.const("shape_flat", np.asarray([0, F * T], np.int64))
    net.nodes.append(node("Reshape", [cur, "shape_flat"], ["rec"], name="to_columns"))
    net.layers.append(("reshape", "rec", [cur], dict(shape=(F * T,))))
    net.nodes.append(node("Sub", ["X", "rec"], ["diff"], name="diff"))
    net.layers.append(("sub", "diff", ["X", "rec"], {}))
    net.nodes.append(node("ReduceSumSquare", ["diff"], ["err"], [attr_ints("axes", [1]), attr_i("keepdims", 0)], name="error"))
    net.layers.append(("sumsquare", "err", ["diff"], {}))
    return net.finish("conv1d_autoencoder", value_info("X", ["N", T * F]), "err", ["N"], opset=13, extra={"in_shape": (T * F,)})


def unet_small(in_ch: int = 3, out_ch: int = 3, size: int = 16, base: int = 8, seed: int = 47, norm: str | None = None, groups: int = 4) -> tuple[bytes, dict]:
    """Two-level U-Net: stride-2 stem and encoder convolutions, ConvTranspose k2 s2 up, a Concat skip, and a ConvTranspose k2 s2 head back to
    the input's resolution.  norm = "group": GroupNormalization (opset 21, `groups` groups) + SiLU in place of every bare activation."""
    if norm == "group":
        return _unet_small_group(in_ch, out_ch, size, base, seed, groups)
    if norm is not None:
        raise ValueError(norm)
    net = _DecoderNet(seed)
    e1 = net.act(net.conv("X", in_ch, base, 3, 2, 1), "Relu")             # size / 2
    e2 = net.act(net.conv(e1, base, 2 * base, 3, 2, 1), "Relu")           # size / 4
    bott = net.act(net.conv(e2, 2 * base, 2 * base, 3, 1, 1), "Relu")
    up = net.act(net.convt(bott, 2 * base, base, 2, 2), "Relu")           # size / 2
    dec = net.act(net.conv(net.concat([up, e1]), 2 * base, base, 3, 1, 1), "Relu")
    head = net.convt(dec, base, out_ch, 2, 2)                             # size
    return net.finish("unet_small", value_info("X", ["N", in_ch, size, size]), head, ["N", out_ch, size, size], extra={"in_shape": (in_ch, size, size)})


def upsample_decoder(latent: Sequence[int] = (8, 4, 4), out_ch: int = 3, seed: int = 53) -> tuple[bytes, dict]:
    """The nn.Upsample spelling of a decoder: (Resize nearest x2, asymmetric / floor -> Conv 3x3) twice."""
    c, h, w = latent
    net = _DecoderNet(seed)
    cur = net.resize("X", 4, scales=(2.0, 2.0))
    cur = net.act(net.conv(cur, c, c, 3, 1, 1), "Relu")
    cur = net.resize(cur, 4, scales=(2.0, 2.0))
    cur = net.conv(cur, c, out_ch, 3, 1, 1)
    return net.finish("upsample_decoder", value_info("X", ["N", c, h, w]), cur, ["N", out_ch, 4 * h, 4 * w], extra={"in_shape": (c, h, w)})


# ------------------------------------------------------------------------------------------
# InstanceNormalization / GroupNormalization
# ------------------------------------------------------------------------------------------
def spatialnorm_reference(x, groups: int, gamma, beta, eps: float) -> np.ndarray:
    """x [N, C, ...] normalised over each of `groups` channel groups (and every spatial position), then gamma[c] * . + beta[c]: float64,
    the biased variance, as InstanceNormalization (groups = C) and GroupNormalization define it."""
    x = np.asarray(x, np.float64)
    n, c = x.shape[:2]
    g = x.reshape(n, groups, -1)
    mean = g.mean(axis=2, keepdims=True)
    d = g - mean
    var = (d * d).mean(axis=2, keepdims=True)
    y = (d / np.sqrt(var + float(eps))).reshape(x.shape)
    sh = (1, c) + (1,) * (x.ndim - 2)
    return y * np.asarray(gamma, np.float64).reshape(sh) + np.asarray(beta, np.float64).reshape(sh)


def spatial_norm_model(c: int = 8, groups: int = 8, hw=(5, 7), op: str = "InstanceNormalization", form: str = "op21", act: str | None = None, pre: bool = False,
                       post: bool = False, offset: float = 0.0, seed: int = 7, inner=None, back: str = "const", affine: str = "mul_add", eps: float = 1e-5,
                       name: str = "norm") -> tuple[bytes, dict]:
    """One normalisation layer `name` on [N, c, H, W] (hw = (L,): [N, c, L]).  op "InstanceNormalization" (groups is then c), or
    "GroupNormalization" in `form` "op18" / "op21" / "exporter" (_DecoderNet.gnorm).  act: None, "Silu" (Sigmoid + Mul) or an activation
    operator.  pre / post: the identity 1x1 Conv / ConvTranspose of conv_transpose_model around it, which put the layer on channel-quad
    tensors.  offset: the common offset of the inputs spatial_norm_inputs draws.  Returns (model, spec) for decoder_reference."""
    one_d = len(hw) == 1
    net = _DecoderNet(seed)
    cur = "X"
    eye = np.eye(c, dtype=np.float32)[:, :, None, None]
    if pre:
        cur = net.conv(cur, c, c, 1, 1, 0, bias=False, w=eye, one_d=one_d)
    if op == "InstanceNormalization":
        cur, opset = net.inorm(cur, c, eps, name=name), 13
    elif op == "GroupNormalization":
        cur = net.gnorm(cur, c, groups, form, inner, eps, name=name, back=back, affine=affine, x_shape=(c,) + tuple(hw))
        opset = {"op18": 18, "op21": 21, "exporter": 13}[form]
    else:
        raise ValueError(op)
    if act == "Silu":
        cur = net.silu(cur)
    elif act:
        cur = net.act(cur, act)
    if post:
        cur = net.convt(cur, c, c, 1, 1, 0, bias=False, w=eye, one_d=one_d)
    shape = (c,) + tuple(hw)
    return net.finish("spatial_norm", value_info("X", ["N"] + list(shape)), cur, ["N"] + list(shape), opset=opset,
                      extra={"in_shape": shape, "out_shape": shape, "offset": float(offset)})


def spatial_norm_inputs(spec: dict, rows: int, seed: int = 0) -> np.ndarray:
    """x = offset + U(-1, 1), f32"""
    rng = np.random.default_rng(seed)
    return (spec.get("offset", 0.0) + rng.uniform(-1, 1, size=(rows,) + tuple(spec["in_shape"]))).astype(np.float32)


def style_net_small(size: int = 16, base: int = 8, seed: int = 59) -> tuple[bytes, dict]:
    """A fast-neural-style transformer in small: Conv 3x3 -> InstanceNormalization -> Relu, two residual blocks (Conv -> InstanceNorm -> Relu ->
    Conv -> InstanceNorm, + the block's input), Upsample x2 + Conv 3x3 stride 2 -> InstanceNorm -> Relu, and a 3x3 stride-1 ConvTranspose (a
    convolution that may store the served NCHW image itself) back to 3 x size x size."""
    net = _DecoderNet(seed)
    cur = net.act(net.inorm(net.conv("X", 3, base, 3, 1, 1), base), "Relu")
    for _ in range(2):
        h = net.act(net.inorm(net.conv(cur, base, base, 3, 1, 1), base), "Relu")
        h = net.inorm(net.conv(h, base, base, 3, 1, 1), base)
        cur = net.add(h, cur)
    cur = net.resize(cur, 4, scales=(2.0, 2.0))
    cur = net.act(net.inorm(net.conv(cur, base, base, 3, 2, 1), base), "Relu")
    cur = net.convt(cur, base, 3, 3, 1, 1)
    shape = (3, size, size)
    return net.finish("style_net_small", value_info("X", ["N"] + list(shape)), cur, ["N"] + list(shape), extra={"in_shape": shape})


def _unet_small_group(in_ch, out_ch, size, base, seed, groups) -> tuple[bytes, dict]:
    net = _DecoderNet(seed)
    gs = lambda x, c: net.silu(net.gnorm(x, c, groups, "op21"))
    e1 = gs(net.conv("X", in_ch, base, 3, 2, 1), base)                    # size / 2
    e2 = gs(net.conv(e1, base, 2 * base, 3, 2, 1), 2 * base)              # size / 4
    bott = gs(net.conv(e2, 2 * base, 2 * base, 3, 1, 1), 2 * base)
    up = gs(net.convt(bott, 2 * base, base, 2, 2), base)                  # size / 2
    dec = gs(net.conv(net.concat([up, e1]), 2 * base, base, 3, 1, 1), base)
    head = net.convt(dec, base, out_ch, 2, 2)                             # size
    return net.finish("unet_small_group", value_info("X", ["N", in_ch, size, size]), head, ["N", out_ch, size, size], opset=21, extra={"in_shape": (in_ch, size, size)})


# ------------------------------------------------------------------------------------------
# Vision Transformers: the crossing from an [N, C, H, W] tensor to a token window [N, T, E] (Tokens step) and the models around it
# ------------------------------------------------------------------------------------------

def token_nodes(nodes: list, inits: list, src: str, c: int, hw, prefix=None, pos=None, view: str = "flatten", expand: str = "subgraph",
                batch: int | str = "N", batch_from: str = "X", p: str = "tok_", pos_rank: int = 3, prefix_behind: bool = False,
                second_reader: bool = False) -> str:
    """Appends the Hugging Face spelling of the crossing behind the [N, c, *hw] value `src` and returns the name of the [N, P + S, c] result:
    the view -- "flatten" (Flatten(axis = 2), torch's flatten(2) kept as one node), "reshape" (Reshape to the constant [0, c, S]) or
    "shape_subgraph" (Reshape to Shape(src)[0:2] ++ [-1], what the exporter writes for flatten(2)) --, Transpose(0, 2, 1), then per array of
    `prefix` (each [p, c]: class / distillation tokens) an Expand -- expand = "subgraph" (target Shape(batch_from) -> Gather(0) -> Unsqueeze
    -> Concat with [p, c]), "literal" (a constant target, with a fixed `batch`) or "none" (the [1, p, c] constant itself) -- joined in front
    by one Concat(axis = 1), then Add(pos [1, P + S, c], or [P + S, c] with pos_rank = 2).  prefix_behind: the constants behind the tokens.
    second_reader: the result is Max(tokens + pos, tokens), so that the position Add is not the only reader of the tokens."""
    i64 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.int64)))  # noqa: E731
    f32 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.float32)))  # noqa: E731
    S = int(np.prod(hw))
    if view == "flatten":
        nodes.append(node("Flatten", [src], [p + "view"], [attr_i("axis", 2)], name=p + "flatten"))
    elif view == "reshape":
        i64(p + "view_shape", [0, c, S])
        nodes.append(node("Reshape", [src, p + "view_shape"], [p + "view"], name=p + "reshape"))
    elif view == "shape_subgraph":
        i64(p + "b0", [0]); i64(p + "b2", [2]); i64(p + "m1", [-1])  # noqa: E702
        nodes += [node("Shape", [src], [p + "src_shape"]), node("Slice", [p + "src_shape", p + "b0", p + "b2", p + "b0"], [p + "nc"]),
                  node("Concat", [p + "nc", p + "m1"], [p + "view_shape"], [attr_i("axis", 0)]),
                  node("Reshape", [src, p + "view_shape"], [p + "view"], name=p + "reshape")]
    elif view != "none":
        raise ValueError(view)
    cur = p + "seq"
    nodes.append(node("Transpose", [src if view == "none" else p + "view"], [cur], [attr_ints("perm", [0, 2, 1])], name=p + "transpose"))
    parts = []
    for j, rows in enumerate(prefix or ()):
        rows = np.asarray(rows, dtype=np.float32).reshape(1, -1, np.asarray(rows).shape[-1])
        f32(f"{p}cls{j}", rows)
        if expand == "none":
            parts.append(f"{p}cls{j}")
            continue
        if expand == "subgraph":
            if j == 0:
                i64(p + "i0", 0); i64(p + "ax0", [0])  # noqa: E702
                nodes += [node("Shape", [batch_from], [p + "in_shape"]), node("Gather", [p + "in_shape", p + "i0"], [p + "n"], [attr_i("axis", 0)]),
                          node("Unsqueeze", [p + "n", p + "ax0"], [p + "n1"])]
            i64(f"{p}pe{j}", list(rows.shape[1:]))
            nodes.append(node("Concat", [p + "n1", f"{p}pe{j}"], [f"{p}target{j}"], [attr_i("axis", 0)]))
        elif expand == "literal":
            i64(f"{p}target{j}", [int(batch), rows.shape[1], rows.shape[2]])
        else:
            raise ValueError(expand)
        nodes.append(node("Expand", [f"{p}cls{j}", f"{p}target{j}"], [f"{p}cls{j}_n"], name=f"{p}expand{j}"))
        parts.append(f"{p}cls{j}_n")
    if parts:
        nodes.append(node("Concat", [cur] + parts if prefix_behind else parts + [cur], [p + "cat"], [attr_i("axis", 1)], name=p + "concat"))
        cur = p + "cat"
    if pos is not None:
        pos = np.asarray(pos, dtype=np.float32)
        f32(p + "pos", pos.reshape((1,) + pos.shape[-2:]) if pos_rank == 3 else pos.reshape(pos.shape[-2:]))
        nodes.append(node("Add", [cur, p + "pos"], [p + "emb"], name=p + "pos_add"))
        if second_reader:
            nodes.append(node("Max", [p + "emb", cur], [p + "both"], name=p + "second_reader"))
        cur = p + "both" if second_reader else p + "emb"
    return cur


def tokens_model(c: int = 8, hw=(4, 4), prefix: int = 0, pos: bool = False, front: str = "relu", view: str = "flatten", expand: str = "subgraph",
                 batch: int | str = "N", seed: int = 5, **kw) -> tuple[bytes, dict]:
    """The Tokens step alone: X [N, c, *hw] -> front -> view -> Transpose(0, 2, 1) [-> Concat(`prefix` expanded constant rows, .)] [-> Add(pos)],
    output [N, prefix + S, c].  front "relu": Relu(X), exact, read in NCHW order; "neg": Neg(X), likewise, and a NaN stays a NaN; "conv": a 1x1 Conv whose weight is twice the identity
    (exact products; the scheduler keeps its result in channel quads when c % 4 == 0).  hw = (L,): the [N, c, L] form.  The constants are
    small integers over 4, so prefix + pos is exact in any order but still exercises the addition.  Returns (model, {"prefix", "pos"})."""
    rng = np.random.default_rng(seed)
    hw = tuple(hw)
    S = int(np.prod(hw))
    nodes, inits = [], []
    if front == "relu":
        nodes.append(node("Relu", ["X"], ["front"], name="front_relu"))
    elif front == "neg":
        nodes.append(node("Neg", ["X"], ["front"], name="front_neg"))
    elif front == "conv":
        w = 2.0 * np.eye(c, dtype=np.float32).reshape((c, c) + (1,) * len(hw))
        inits.append(tensor("front_w", w))
        nodes.append(node("Conv", ["X", "front_w"], ["front"], [attr_ints("kernel_shape", [1] * len(hw))], name="front_conv"))
    else:
        raise ValueError(front)
    cls = (rng.integers(-64, 64, (prefix, c)) / 4.0).astype(np.float32) if prefix else None
    table = (rng.integers(-64, 64, (prefix + S, c)) / 4.0).astype(np.float32) if pos else None
    out = token_nodes(nodes, inits, "front", c, hw, [cls[j:j + 1] for j in range(prefix)] if prefix else None, table, view=view, expand=expand, batch=batch, **kw)
    blob = model("tokens", nodes, inits, [value_info("X", [batch, c] + list(hw))], [value_info(out, [batch, prefix + S, c])], opset=13)
    return blob, {"c": c, "hw": hw, "prefix": cls, "pos": table, "front": front, "second_reader": bool(kw.get("second_reader"))}


def tokens_reference(spec: dict, x) -> np.ndarray:
    """What tokens_model computes, in float32 numpy: exact movement and one IEEE addition per element."""
    x = np.asarray(x, dtype=np.float32)
    n, c = x.shape[:2]
    f = np.maximum(x, 0) if spec["front"] == "relu" else -x if spec["front"] == "neg" else np.float32(2.0) * x
    tok = f.reshape(n, c, -1).transpose(0, 2, 1)
    if spec["prefix"] is not None:
        tok = np.concatenate([np.broadcast_to(spec["prefix"][None], (n,) + spec["prefix"].shape), tok], axis=1)
    if spec["pos"] is None:
        return np.ascontiguousarray(tok)
    emb = (tok + spec["pos"][None]).astype(np.float32)
    return np.maximum(emb, tok) if spec.get("second_reader") else emb


def vit_spec(img=(3, 16, 16), patch: int = 4, E: int = 32, h: int = 4, ff: int = 64, layers: int = 2, classes: int = 5, prefix: int = 1,
             weight_scale: float = 1.0, seed: int = 33) -> dict:
    """A seeded ViT / DeiT in the Hugging Face spelling: a patch x patch stride-patch Conv with bias img[0] -> E, `prefix` class /
    distillation tokens, a position table [prefix + S, E], `layers` pre-norm encoder layers with Erf GELU (transformer_spec), the final
    LayerNorm and a classifier on the first token."""
    rng = np.random.default_rng(seed)
    c, H, W = img
    S = (H // patch) * (W // patch)
    k = weight_scale / np.sqrt(c * patch * patch)
    enc = transformer_spec(T=prefix + S, F=E, E=E, h=h, ff=ff, layers=layers, norm_first=True, act="Gelu", outputs=classes, weight_scale=weight_scale, seed=seed + 1)
    enc.update(Win=None, bin=None, pos=None)
    return {"img": tuple(img), "patch": patch, "E": E, "grid": (H // patch, W // patch), "enc": enc,
            "patch_W": rng.uniform(-k, k, (E, c, patch, patch)).astype(np.float32), "patch_b": rng.uniform(-k, k, (E,)).astype(np.float32),
            "cls": (0.5 * rng.standard_normal((prefix, E))).astype(np.float32), "pos": (0.5 * rng.standard_normal((prefix + S, E))).astype(np.float32)}


def vit_from_spec(spec: dict, view: str = "flatten", expand: str = "subgraph", batch: int | str = "N", second_reader: bool = False,
                  heads: Sequence[str] = ("first",), **kw) -> bytes:
    """The ONNX model of a vit_spec() dict, input X [N, C, H, W]: Conv(patch, with bias) -> view -> Transpose -> Concat(expanded class tokens, .) ->
    Add(position table) -> transformer_from_spec(spec["enc"], separate Q / K / V) -> the first token -> classifier (output "first").
    view, expand, second_reader: token_nodes (second_reader changes what the model computes: for plan checks).  kw: transformer_from_spec (gelu = "decomposed", shape = "subgraph" ...)."""
    c, H, W = spec["img"]
    pt, E = spec["patch"], spec["E"]
    nodes = [node("Conv", ["X", "patch_W", "patch_b"], ["patches"], [attr_ints("kernel_shape", [pt, pt]), attr_ints("strides", [pt, pt])], name="patch_embed")]
    inits = [tensor("patch_W", spec["patch_W"]), tensor("patch_b", spec["patch_b"])]
    P = spec["cls"].shape[0]
    x = token_nodes(nodes, inits, "patches", E, spec["grid"], [spec["cls"][j:j + 1] for j in range(P)], spec["pos"], view=view, expand=expand, batch=batch,
                    second_reader=second_reader)
    return transformer_from_spec(spec["enc"], heads=heads, front=(nodes, inits, x, [value_info("X", [batch, c, H, W])]), **kw)


def vit_reference(spec: dict, x, heads: Sequence[str] = ("first",)) -> dict:
    """float64 numpy restatement of vit_from_spec(spec): x [N, C, H, W] -> {output name: array}."""
    pt = spec["patch"]
    x = np.asarray(x, dtype=np.float64).reshape((-1,) + tuple(spec["img"]))
    f = _conv_taps(x, np.asarray(spec["patch_W"], np.float64), (pt, pt), (0, 0, 0, 0), (1, 1), 1, 0.0) + np.asarray(spec["patch_b"], np.float64).reshape(1, -1, 1, 1)
    n, E = f.shape[:2]
    tok = f.reshape(n, E, -1).transpose(0, 2, 1)
    tok = np.concatenate([np.broadcast_to(np.asarray(spec["cls"], np.float64)[None], (n,) + spec["cls"].shape), tok], axis=1) + np.asarray(spec["pos"], np.float64)[None]
    return transformer_reference(spec["enc"], tok, heads)


def cnn_stem_encoder_spec(img=(3, 12, 12), base: int = 8, E: int = 16, h: int = 2, ff: int = 32, classes: int = 4, weight_scale: float = 1.0, seed: int = 61) -> dict:
    """A CNN stem in front of an encoder: Conv 3x3 stride 2 (img[0] -> base) -> Relu -> Conv 3x3 stride 2 (base -> E) -> tokens (no class
    token) -> position table -> one post-norm encoder layer (Relu) -> mean over time -> classifier."""
    rng = np.random.default_rng(seed)
    c, H, W = img
    g = ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2
    S = g[0] * g[1]
    enc = transformer_spec(T=S, F=E, E=E, h=h, ff=ff, layers=1, norm_first=False, act="Relu", outputs=classes, weight_scale=weight_scale, seed=seed + 1)
    enc.update(Win=None, bin=None, pos=None)
    u = lambda shape, fan: rng.uniform(-weight_scale / np.sqrt(fan), weight_scale / np.sqrt(fan), shape).astype(np.float32)  # noqa: E731
    return {"img": tuple(img), "grid": g, "E": E, "enc": enc, "W1": u((base, c, 3, 3), 9 * c), "b1": u((base,), 9 * c), "W2": u((E, base, 3, 3), 9 * base),
            "b2": u((E,), 9 * base), "pos": (0.5 * rng.standard_normal((S, E))).astype(np.float32)}


def cnn_stem_encoder_from_spec(spec: dict, view: str = "reshape", **kw) -> bytes:
    c, H, W = spec["img"]
    conv = lambda x, w, b, out, name: node("Conv", [x, w, b], [out], [attr_ints("kernel_shape", [3, 3]), attr_ints("strides", [2, 2]), attr_ints("pads", [1, 1, 1, 1])], name=name)  # noqa: E731
    nodes = [conv("X", "W1", "b1", "c1", "stem1"), node("Relu", ["c1"], ["r1"], name="stem_relu"), conv("r1", "W2", "b2", "c2", "stem2")]
    inits = [tensor(k, spec[k]) for k in ("W1", "b1", "W2", "b2")]
    x = token_nodes(nodes, inits, "c2", spec["E"], spec["grid"], None, spec["pos"], view=view)
    return transformer_from_spec(spec["enc"], heads=("mean",), front=(nodes, inits, x, [value_info("X", ["N", c, H, W])]), **kw)


def cnn_stem_encoder_reference(spec: dict, x) -> dict:
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    x = f64(x).reshape((-1,) + tuple(spec["img"]))
    conv = lambda a, w, b: _conv_taps(a, f64(w), (2, 2), (1, 1, 1, 1), (1, 1), 1, 0.0) + f64(b).reshape(1, -1, 1, 1)  # noqa: E731
    f = conv(np.maximum(conv(x, spec["W1"], spec["b1"]), 0.0), spec["W2"], spec["b2"])
    n, E = f.shape[:2]
    return transformer_reference(spec["enc"], f.reshape(n, E, -1).transpose(0, 2, 1) + f64(spec["pos"])[None], ("mean",))


# ------------------------------------------------------------------------------------------
# ConvNeXt: LayerNorm over the channel axis at each pixel (ChannelNorm step) and the channels-last detour around it
# ------------------------------------------------------------------------------------------
def channelnorm_reference(x, gamma, beta, eps: float) -> np.ndarray:
    """x [N, C, H, W] normalised over the C channels at each pixel (the biased variance), then gamma[c] * . + beta[c] (beta None: none): float64."""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True)
    y = d / np.sqrt(var + float(eps)) * np.asarray(gamma, np.float64).reshape(1, -1, 1, 1)
    return y if beta is None else y + np.asarray(beta, np.float64).reshape(1, -1, 1, 1)


def _gelu64(a):
    from math import erf
    return 0.5 * a * (1.0 + np.vectorize(erf)(a / math.sqrt(2.0)))


class _ConvNextNet:
    """Appends the nodes of ConvNeXt layers in one of the spellings exporters write.  Values are named [N, C, H, W] tensors between layers;
    style "torchvision" / "hf" take the channels-last detour (Transpose(0,2,3,1) ... Transpose(0,3,1,2)), "nchw" spells the same layers
    with the channels-first norm and 1x1 Conv nodes."""

    def __init__(self, dtype=np.float32):
        self.nodes, self.inits, self.dtype, self.count = [], [], dtype, 0

    def f(self, name, v):
        self.inits.append(tensor(name, np.asarray(v, dtype=self.dtype)))
        return name

    def i64(self, name, v):
        self.inits.append(tensor(name, np.asarray(v, dtype=np.int64)))
        return name

    def op(self, op, ins, out, attrs=(), name=None):
        self.nodes.append(node(op, list(ins), [out], list(attrs), name=name or out))
        return out

    def to_last(self, x, p):
        return self.op("Transpose", [x], p + "_nhwc", [attr_ints("perm", [0, 2, 3, 1])], name=p + "_to_last")

    def to_first(self, x, p, out=None):
        return self.op("Transpose", [x], out or p + "_nchw", [attr_ints("perm", [0, 3, 1, 2])], name=p + "_to_first")

    def norm_op(self, x_last, g, b, eps, p, axis=-1, outputs=1):
        """LayerNormalization on a channels-last value; the result is channels-last"""
        ins = [x_last, self.f(p + "_g", g)] + ([self.f(p + "_b", b)] if b is not None else [])
        outs = [p + "_ln"] + [p + "_mean", p + "_isd"][:outputs - 1]
        self.nodes.append(node("LayerNormalization", ins, outs, [attr_i("axis", axis), attr_f("epsilon", eps)], name=p + "_ln"))
        return outs[0]

    def norm_first(self, x, g, b, eps, p, square="pow"):
        """Hugging Face's channels-first ConvNextLayerNorm on an [N, C, H, W] value"""
        c = len(g)
        self.i64(p + "_ax", [1])
        self.f(p + "_eps", np.asarray(eps))
        ax = [attr_ints("axes", [1]), attr_i("keepdims", 1)]
        self.op("ReduceMean", [x], p + "_mu", ax, name=p + "_mean")
        self.op("Sub", [x, p + "_mu"], p + "_d", name=p + "_sub")
        if square == "pow":
            self.op("Pow", [p + "_d", self.f(p + "_two", np.asarray(2.0))], p + "_sq", name=p + "_pow")
        else:
            self.op("Mul", [p + "_d", p + "_d"], p + "_sq", name=p + "_square")
        self.op("ReduceMean", [p + "_sq"], p + "_var", ax, name=p + "_varmean")
        self.op("Add", [p + "_var", p + "_eps"], p + "_ve", name=p + "_addeps")
        self.op("Sqrt", [p + "_ve"], p + "_sd", name=p + "_sqrt")
        cur = self.op("Div", [p + "_d", p + "_sd"], p + "_nrm", name=p + "_div")
        cur = self.op("Mul", [self.f(p + "_g", np.asarray(g).reshape(c, 1, 1)), cur], p + "_sc", name=p + "_gamma")
        if b is not None:
            cur = self.op("Add", [cur, self.f(p + "_b", np.asarray(b).reshape(c, 1, 1))], p + "_cf", name=p + "_beta")
        return cur

    def norm2d(self, x, g, b, eps, p, style):
        """the norm of an [N, C, H, W] value, [N, C, H, W] again: torchvision's LayerNorm2d or the channels-first chain"""
        if style == "torchvision":
            return self.to_first(self.norm_op(self.to_last(x, p), g, b, eps, p), p)
        return self.norm_first(x, g, b, eps, p)

    def gelu(self, x, p, form):
        if form == "op":
            return self.op("Gelu", [x], p + "_gelu")
        self.f(p + "_sqrt2", np.asarray(math.sqrt(2.0))); self.f(p + "_one", np.asarray(1.0)); self.f(p + "_half", np.asarray(0.5))  # noqa: E702
        self.op("Div", [x, p + "_sqrt2"], p + "_g0")
        self.op("Erf", [p + "_g0"], p + "_g1")
        self.op("Add", [p + "_g1", p + "_one"], p + "_g2")
        self.op("Mul", [x, p + "_g2"], p + "_g3")
        return self.op("Mul", [p + "_g3", p + "_half"], p + "_gelu")

    def block(self, x, L, eps, p, style, gelu="op"):
        """depthwise 7x7 -> norm -> Linear 4C -> GELU -> Linear C -> layer scale -> + x.  L: dw_W [C,1,7,7], dw_b, g, b, W1 [C,4C], b1, W2 [4C,C], b2, ls [C] | None"""
        c = len(L["g"])
        dw = self.op("Conv", [x, self.f(p + "_dwW", L["dw_W"]), self.f(p + "_dwb", L["dw_b"])], p + "_dw",
                     [attr_ints("kernel_shape", [7, 7]), attr_ints("pads", [3, 3, 3, 3]), attr_i("group", c)])
        if style == "nchw":
            h = self.norm_first(dw, L["g"], L["b"], eps, p + "_norm")
            k1 = [attr_ints("kernel_shape", [1, 1])]
            h = self.op("Conv", [h, self.f(p + "_W1", np.asarray(L["W1"]).T.reshape(4 * c, c, 1, 1)), self.f(p + "_b1", L["b1"])], p + "_fc1", k1)
            h = self.gelu(h, p, gelu)
            h = self.op("Conv", [h, self.f(p + "_W2", np.asarray(L["W2"]).T.reshape(c, 4 * c, 1, 1)), self.f(p + "_b2", L["b2"])], p + "_fc2", k1)
            if L.get("ls") is not None:
                h = self.op("Mul", [self.f(p + "_ls", np.asarray(L["ls"]).reshape(c, 1, 1)), h], p + "_scaled")
            return self.op("Add", [x, h], p + "_out", name=p + "_residual")
        h = self.norm_op(self.to_last(dw, p), L["g"], L["b"], eps, p + "_norm")
        h = self.op("Add", [self.op("MatMul", [h, self.f(p + "_W1", L["W1"])], p + "_mm1"), self.f(p + "_b1", L["b1"])], p + "_fc1")
        h = self.gelu(h, p, gelu)
        h = self.op("Add", [self.op("MatMul", [h, self.f(p + "_W2", L["W2"])], p + "_mm2"), self.f(p + "_b2", L["b2"])], p + "_fc2")
        if style == "hf":
            if L.get("ls") is not None:
                h = self.op("Mul", [self.f(p + "_ls", L["ls"]), h], p + "_scaled")
            h = self.to_first(h, p)
        else:
            h = self.to_first(h, p)
            if L.get("ls") is not None:
                h = self.op("Mul", [self.f(p + "_ls", np.asarray(L["ls"]).reshape(c, 1, 1)), h], p + "_scaled")
        return self.op("Add", [x, h], p + "_out", name=p + "_residual")


def _block_params(rng, c, scale=1.0, layer_scale=True):
    u = lambda shape, fan: (rng.uniform(-1, 1, shape) * scale / math.sqrt(fan)).astype(np.float32)  # noqa: E731
    return {"dw_W": u((c, 1, 7, 7), 49), "dw_b": u((c,), 49), "g": rng.uniform(0.5, 1.5, c).astype(np.float32), "b": rng.uniform(-0.5, 0.5, c).astype(np.float32),
            "W1": u((c, 4 * c), c), "b1": u((4 * c,), c), "W2": u((4 * c, c), 4 * c), "b2": u((c,), 4 * c),
            "ls": rng.uniform(0.25, 1.0, c).astype(np.float32) if layer_scale else None}


def _block_reference(x, L, eps):
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    c = x.shape[1]
    h = _conv_taps(x, f64(L["dw_W"]), (1, 1), (3, 3, 3, 3), (1, 1), c, 0.0) + f64(L["dw_b"]).reshape(1, -1, 1, 1)
    h = channelnorm_reference(h, L["g"], L["b"], eps).transpose(0, 2, 3, 1)
    h = _gelu64(h @ f64(L["W1"]) + f64(L["b1"])) @ f64(L["W2"]) + f64(L["b2"])
    if L.get("ls") is not None:
        h = h * f64(L["ls"])
    return x + h.transpose(0, 3, 1, 2)


def channel_norm_model(c: int = 8, hw=(5, 7), spelling: str = "nhwc_op", act: str | None = None, front: str = "relu", eps: float = 1e-6, bias: bool = True,
                       post_affine: bool = False, square: str = "pow", offset: float = 0.0, integer: bool = False, seed: int = 7) -> tuple[bytes, dict]:
    """One norm over the channels of [N, c, H, W] behind `front` -- "relu": Relu(X), an NCHW tensor; "conv": an identity 1x1 Conv in front
    and an identity 1x1 ConvTranspose behind, which put the layer on channel-quad tensors where c % 4 == 0 (exact: X passes unchanged).
    spelling "nhwc_op": Transpose(0,2,3,1) -> LayerNormalization -> [post_affine: Mul([c]) -> Add([c])] -> [act] -> Transpose(0,3,1,2), all
    on the channels-last value; "layernorm2d" (torchvision): Transpose -> LayerNormalization -> Transpose back -> [Mul([c,1,1]) -> Add] -> [act];
    "channels_first" (Hugging Face): the ReduceMean(axes = [1]) chain (square: "pow" | "mul") -> [Mul -> Add] -> [act].  integer: gamma and
    beta are small integers over 8.  Returns (model, spec) for channel_norm_reference."""
    rng = np.random.default_rng(seed)
    H, W = hw
    if integer:
        g, b = (rng.integers(1, 16, c) / 8.0).astype(np.float32), (rng.integers(-16, 16, c) / 8.0).astype(np.float32)
    else:
        g, b = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)
    if not bias:
        b = None
    g2, b2 = (rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)) if post_affine else (None, None)
    net = _ConvNextNet()
    eye = np.eye(c, dtype=np.float32).reshape(c, c, 1, 1)
    if front == "relu":
        cur = net.op("Relu", ["X"], "front", name="front_relu")
    elif front == "conv":
        cur = net.op("Conv", ["X", net.f("front_w", eye)], "front", [attr_ints("kernel_shape", [1, 1])], name="front_conv")
    else:
        raise ValueError(front)
    last = spelling == "nhwc_op"
    if spelling in ("nhwc_op", "layernorm2d"):
        cur = net.norm_op(net.to_last(cur, "norm"), g, b, eps, "norm")
        if not last:
            cur = net.to_first(cur, "norm")
    elif spelling == "channels_first":
        cur = net.norm_first(cur, g, b, eps, "norm", square)
    else:
        raise ValueError(spelling)
    if post_affine:
        sh = (c,) if last else (c, 1, 1)
        cur = net.op("Mul", [cur, net.f("post_g", g2.reshape(sh))], "post_mul")
        cur = net.op("Add", [cur, net.f("post_b", b2.reshape(sh))], "post_add")
    if act:
        cur = net.op(act, [cur], "act")
    if last:
        cur = net.to_first(cur, "norm_back")
    if front == "conv":
        cur = net.op("ConvTranspose", [cur, net.f("back_w", eye)], "back", [attr_ints("strides", [1, 1]), attr_ints("pads", [0, 0, 0, 0])], name="back_convt")
    blob = model("channel_norm", net.nodes, net.inits, [value_info("X", ["N", c, H, W])], [value_info(cur, ["N", c, H, W])], opset=20)
    return blob, {"c": c, "hw": (H, W), "in_shape": (c, H, W), "gamma": g, "beta": b, "eps": float(np.float32(eps)), "post": (g2, b2), "act": act, "front": front,
                  "offset": float(offset)}


def channel_norm_inputs(spec: dict, rows: int, seed: int = 0) -> np.ndarray:
    """x = offset + U(-1, 1), f32"""
    rng = np.random.default_rng(seed)
    return (spec.get("offset", 0.0) + rng.uniform(-1, 1, size=(rows,) + tuple(spec["in_shape"]))).astype(np.float32)


def channel_norm_reference(spec: dict, x) -> np.ndarray:
    """What channel_norm_model computes, in float64"""
    x = np.asarray(x, np.float64).reshape((-1,) + tuple(spec["in_shape"]))
    f = np.maximum(x, 0.0) if spec["front"] == "relu" else x
    y = channelnorm_reference(f, spec["gamma"], spec["beta"], spec["eps"])
    if spec["post"][0] is not None:
        y = y * np.asarray(spec["post"][0], np.float64).reshape(1, -1, 1, 1) + np.asarray(spec["post"][1], np.float64).reshape(1, -1, 1, 1)
    if spec["act"] == "Relu":
        y = np.maximum(y, 0.0)
    elif spec["act"] == "Sigmoid":
        y = 1.0 / (1.0 + np.exp(-y))
    elif spec["act"]:
        raise ValueError(spec["act"])
    return y


def convnext_block_model(c: int = 8, hw=(7, 7), style: str = "torchvision", gelu: str = "op", layer_scale: bool = True, eps: float = 1e-6, seed: int = 11,
                         weight_scale: float = 1.0) -> tuple[bytes, dict]:
    """One ConvNeXt block on [N, c, H, W] between a 1x1 Conv with bias (so that the block reads a tensor a step wrote, in channel quads when
    c % 4 == 0) and an identity 1x1 ConvTranspose (which stores the served NCHW tensor).  style: "torchvision" ([c,1,1] layer scale after the
    permute back), "hf" ([c] layer scale before it), "nchw" (the same block with the channels-first norm and Conv 1x1 nodes, no Transpose).
    gelu: "op" | "decomposed".  Returns (model, spec) for convnext_block_reference."""
    rng = np.random.default_rng(seed)
    H, W = hw
    stem_W = (rng.uniform(-1, 1, (c, c, 1, 1)) * weight_scale / math.sqrt(c)).astype(np.float32)
    stem_b = (rng.uniform(-1, 1, c) * weight_scale).astype(np.float32)
    L = _block_params(rng, c, weight_scale, layer_scale)
    net = _ConvNextNet()
    cur = net.op("Conv", ["X", net.f("stem_W", stem_W), net.f("stem_b", stem_b)], "stem", [attr_ints("kernel_shape", [1, 1])])
    cur = net.block(cur, L, eps, "blk", style, gelu)
    cur = net.op("ConvTranspose", [cur, net.f("back_w", np.eye(c, dtype=np.float32).reshape(c, c, 1, 1))], "back", [attr_ints("strides", [1, 1]), attr_ints("pads", [0, 0, 0, 0])])
    blob = model("convnext_block", net.nodes, net.inits, [value_info("X", ["N", c, H, W])], [value_info(cur, ["N", c, H, W])], opset=20)
    return blob, {"c": c, "hw": (H, W), "in_shape": (c, H, W), "stem_W": stem_W, "stem_b": stem_b, "block": L, "eps": float(np.float32(eps))}


def convnext_block_reference(spec: dict, x) -> np.ndarray:
    x = np.asarray(x, np.float64).reshape((-1,) + tuple(spec["in_shape"]))
    f = _conv_taps(x, np.asarray(spec["stem_W"], np.float64), (1, 1), (0, 0, 0, 0), (1, 1), 1, 0.0) + np.asarray(spec["stem_b"], np.float64).reshape(1, -1, 1, 1)
    return _block_reference(f, spec["block"], spec["eps"])


def convnext_spec(img=(3, 32, 32), widths: Sequence[int] = (8, 16), depths: Sequence[int] = (1, 1), classes: int = 5, weight_scale: float = 1.0,
                  layer_scale: bool = True, eps: float = 1e-6, seed: int = 71) -> dict:
    """A seeded ConvNeXt in small: stem Conv k4 s4 + LayerNorm2d; per stage `depths[i]` blocks of width `widths[i]` (depthwise 7x7 -> norm ->
    Linear 4C -> GELU -> Linear C -> layer scale -> residual); LayerNorm2d + Conv k2 s2 between stages; global pool -> norm -> Linear."""
    rng = np.random.default_rng(seed)
    u = lambda shape, fan: (rng.uniform(-1, 1, shape) * weight_scale / math.sqrt(fan)).astype(np.float32)  # noqa: E731
    nrm = lambda c: (rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32))  # noqa: E731
    c0 = img[0]
    spec = {"img": tuple(img), "widths": tuple(widths), "depths": tuple(depths), "classes": classes, "eps": float(np.float32(eps)),
            "stem_W": u((widths[0], c0, 4, 4), 16 * c0), "stem_b": u((widths[0],), 16 * c0), "stem_norm": nrm(widths[0]), "stages": [], "down": []}
    for i, (c, d) in enumerate(zip(widths, depths)):
        if i > 0:
            spec["down"].append({"norm": nrm(widths[i - 1]), "W": u((c, widths[i - 1], 2, 2), 4 * widths[i - 1]), "b": u((c,), 4 * widths[i - 1])})
        spec["stages"].append([_block_params(rng, c, weight_scale, layer_scale) for _ in range(d)])
    spec["head_norm"] = nrm(widths[-1])
    spec["head_W"], spec["head_b"] = u((widths[-1], classes), widths[-1]), u((classes,), widths[-1])
    return spec


def convnext_norm_count(spec: dict) -> int:
    return 1 + sum(spec["depths"]) + len(spec["down"]) + 1


def convnext_from_spec(spec: dict, style: str = "torchvision", gelu: str = "op", half: bool = False, batch: int | str = "N") -> bytes:
    """The ONNX model of a convnext_spec() dict, input X [N, C, H, W], output "logits" [N, classes].  style "torchvision": every norm is
    Transpose(0,2,3,1) -> LayerNormalization -> Transpose(0,3,1,2) (the head's on the pooled [N, C, 1, 1] tensor), [C,1,1] layer scale; "hf":
    the channels-first chain for the stem and downsampling norms and the head's, the channels-last detour with [C] layer scale in the blocks;
    "nchw": no Transpose anywhere.  half: a float16 graph (float16 input, weights and output)."""
    net = _ConvNextNet(np.float16 if half else np.float32)
    eps, t = spec["eps"], FLOAT16 if half else FLOAT
    cur = net.op("Conv", ["X", net.f("stem_W", spec["stem_W"]), net.f("stem_b", spec["stem_b"])], "stem", [attr_ints("kernel_shape", [4, 4]), attr_ints("strides", [4, 4])])
    nstyle = "torchvision" if style == "torchvision" else "nchw"
    cur = net.norm2d(cur, spec["stem_norm"][0], spec["stem_norm"][1], eps, "stem_norm", nstyle)
    for i, blocks in enumerate(spec["stages"]):
        if i > 0:
            D = spec["down"][i - 1]
            cur = net.norm2d(cur, D["norm"][0], D["norm"][1], eps, f"down{i}_norm", nstyle)
            cur = net.op("Conv", [cur, net.f(f"down{i}_W", D["W"]), net.f(f"down{i}_b", D["b"])], f"down{i}", [attr_ints("kernel_shape", [2, 2]), attr_ints("strides", [2, 2])])
        for j, L in enumerate(blocks):
            cur = net.block(cur, L, eps, f"s{i}b{j}", style, gelu)
    cur = net.op("GlobalAveragePool", [cur], "pool")
    cur = net.norm2d(cur, spec["head_norm"][0], spec["head_norm"][1], eps, "head_norm", nstyle)
    cur = net.op("Flatten", [cur], "flat", [attr_i("axis", 1)])
    net.op("Gemm", [cur, net.f("head_W", spec["head_W"]), net.f("head_b", spec["head_b"])], "logits")
    c, H, W = spec["img"]
    return model("convnext", net.nodes, net.inits, [value_info("X", [batch, c, H, W], t)], [value_info("logits", [batch, spec["classes"]], t)], opset=20)


def convnext_reference(spec: dict, x) -> np.ndarray:
    """float64 numpy restatement of convnext_from_spec(spec): x [N, C, H, W] -> logits [N, classes]."""
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    eps = spec["eps"]
    conv = lambda a, w, b, k: _conv_taps(a, f64(w), (k, k), (0, 0, 0, 0), (1, 1), 1, 0.0) + f64(b).reshape(1, -1, 1, 1)  # noqa: E731
    x = f64(x).reshape((-1,) + tuple(spec["img"]))
    h = channelnorm_reference(conv(x, spec["stem_W"], spec["stem_b"], 4), spec["stem_norm"][0], spec["stem_norm"][1], eps)
    for i, blocks in enumerate(spec["stages"]):
        if i > 0:
            D = spec["down"][i - 1]
            h = conv(channelnorm_reference(h, D["norm"][0], D["norm"][1], eps), D["W"], D["b"], 2)
        for L in blocks:
            h = _block_reference(h, L, eps)
    h = channelnorm_reference(h.mean(axis=(2, 3), keepdims=True), spec["head_norm"][0], spec["head_norm"][1], eps)
    return h.reshape(len(h), -1) @ f64(spec["head_W"]) + f64(spec["head_b"])


# ------------------------------------------------------------------------------------------
# Embedding lookups (Gather of a constant table by runtime indices) in front of MLPs and Transformer encoders
# ------------------------------------------------------------------------------------------

EMBED_SPELLINGS = ("a", "b", "c", "d")


def embedding_spec(cards: Sequence[int] = (7, 11, 5), dims: Sequence[int] | int = (3, 4, 2), numeric: int = 2, hidden: Sequence[int] = (16, 8),
                   outputs: int = 1, seed: int = 71, weight_scale: float = 1.0, table_rank1: bool = False) -> dict:
    """Seeded categorical front end: column j has cards[j] categories and a table [cards[j], dims[j]] (N(0, 1), like nn.Embedding); `numeric`
    f32 columns beside them; an MLP sum(dims) + numeric -> hidden... -> outputs (U(+-1/sqrt(fan_in)) like nn.Linear, scaled by weight_scale;
    hidden = (): no MLP).  With equal dims the spec also holds the one shared table of spelling (b): the tables one below the other and the
    per-column row offsets.  table_rank1: dims are all 1 and the tables have no trailing axis ([V])."""
    rng = np.random.default_rng(seed)
    k = len(cards)
    dims = [int(dims)] * k if isinstance(dims, (int, np.integer)) else [int(d) for d in dims]
    assert len(dims) == k and (not table_rank1 or all(d == 1 for d in dims))
    tables = [rng.standard_normal((int(v), d)).astype(np.float32) for v, d in zip(cards, dims)]
    spec = {"cards": [int(v) for v in cards], "dims": dims, "numeric": int(numeric), "tables": tables, "rank1": bool(table_rank1), "mlp": [], "act": "Relu"}
    if len(set(dims)) == 1:
        spec["shared"] = np.concatenate(tables, axis=0)
        spec["offsets"] = np.concatenate([[0], np.cumsum(spec["cards"])[:-1]]).astype(np.int64)
    widths = [sum(dims) + int(numeric)] + [int(h) for h in hidden] + ([int(outputs)] if hidden else [])
    for i, o in zip(widths[:-1], widths[1:]):
        b = weight_scale / np.sqrt(i)
        spec["mlp"].append((rng.uniform(-b, b, (i, o)).astype(np.float32), rng.uniform(-b, b, (o,)).astype(np.float32)))
    return spec


def from_torch_tabular(module) -> dict:
    """The embedding_spec() dict of a torch.nn model built from nn.Embedding tables (one per categorical column, in module order) and
    nn.Linear layers (in module order, ReLU between them): the first Linear reads cat(embeddings..., numeric columns)."""
    import torch

    embs = [mod for mod in module.modules() if isinstance(mod, torch.nn.Embedding)]
    lins = [mod for mod in module.modules() if isinstance(mod, torch.nn.Linear)]
    assert embs and lins
    tables = [e.weight.detach().cpu().numpy().astype(np.float32).copy() for e in embs]
    dims = [int(t.shape[1]) for t in tables]
    spec = {"cards": [int(t.shape[0]) for t in tables], "dims": dims, "numeric": int(lins[0].in_features) - sum(dims), "tables": tables, "rank1": False,
            "mlp": [(lin.weight.detach().cpu().numpy().astype(np.float32).T.copy(), lin.bias.detach().cpu().numpy().astype(np.float32).copy()) for lin in lins],
            "act": "Relu"}
    assert spec["numeric"] >= 0
    if len(set(dims)) == 1:
        spec["shared"] = np.concatenate(tables, axis=0)
        spec["offsets"] = np.concatenate([[0], np.cumsum(spec["cards"])[:-1]]).astype(np.int64)
    return spec


def embedding_nodes(spec: dict, spelling: str = "a", pick: str = "gather", flatten: str = "reshape", int_type: int = INT64, concat: bool = True,
                    offsets_rank: int = 1, batch: int | str = "N"):
    """The front end of an embedding_spec() as (nodes, initializers, name of its result, dims of the result, graph inputs).
    (a): inputs x_cat [N, k] (int_type) and x_num [N, m]; column j picked by Gather(axis = 1, scalar) (pick "gather") or Slice + Squeeze
         ("slice"), looked up in table j (node 'emb<j>'), the results and x_num joined by Concat -> 'features' [N, sum(d) + m].
    (b): one shared table, x_cat + offsets ([k], or [1, k] with offsets_rank 2) -> Gather (node 'emb') -> [N, k, d]; flatten: "reshape" /
         "flatten" -> [N, k * d] (then Concat with x_num, if any), "window": the [N, k, d] value itself.
    (c): Gather(table 0, ids [N, T = len(cards)]) -> the window [N, T, d] (node 'emb').
    (d): (a) on ONE f32 input X [N, k + m]: column j -> Cast(int_type) -> lookup; the numeric columns are Slice(X, k : k + m).
    concat = False (one lookup, no numeric columns): no Concat node."""
    assert spelling in EMBED_SPELLINGS
    k, m, dims = len(spec["cards"]), spec["numeric"], spec["dims"]
    nodes, inits, inputs = [], [], []
    i64 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.int64)))  # noqa: E731
    table = lambda t: t.reshape(-1) if spec["rank1"] else t  # noqa: E731
    mixed = spelling == "d"
    if mixed:
        inputs.append(value_info("X", [batch, k + m]))
    else:
        inputs.append(value_info("x_cat", [batch, k], int_type))
        if m and spelling != "c":
            inputs.append(value_info("x_num", [batch, m]))
    src = "X" if mixed else "x_cat"
    if spelling in ("a", "d"):
        parts = []
        i64("ax1", [1])
        for j in range(k):
            if pick == "gather":
                i64(f"col{j}_i", j)
                nodes.append(node("Gather", [src, f"col{j}_i"], [f"col{j}"], [attr_i("axis", 1)], name=f"pick{j}"))
            else:
                i64(f"col{j}_b", [j]); i64(f"col{j}_e", [j + 1])  # noqa: E702
                nodes.append(node("Slice", [src, f"col{j}_b", f"col{j}_e", "ax1"], [f"col{j}_s"], name=f"pick{j}"))
                nodes.append(node("Squeeze", [f"col{j}_s", "ax1"], [f"col{j}"], name=f"squeeze{j}"))
            idx = f"col{j}"
            if mixed:
                nodes.append(node("Cast", [idx], [f"col{j}_int"], [attr_i("to", int_type)], name=f"cast{j}"))
                idx = f"col{j}_int"
            inits.append(tensor(f"table{j}", table(spec["tables"][j])))
            nodes.append(node("Gather", [f"table{j}", idx], [f"e{j}"] if not spec["rank1"] else [f"e{j}_flat"], name=f"emb{j}"))
            if spec["rank1"]:  # [N] -> [N, 1] for the Concat
                nodes.append(node("Unsqueeze", [f"e{j}_flat", "ax1"], [f"e{j}"], name=f"unsq{j}"))
            parts.append(f"e{j}")
        if m:
            if mixed:
                i64("num_b", [k]); i64("num_e", [k + m])  # noqa: E702
                nodes.append(node("Slice", ["X", "num_b", "num_e", "ax1"], ["x_num"], name="numeric"))
            parts.append("x_num")
        if len(parts) == 1 and not concat:
            return nodes, inits, parts[0], [batch, dims[0]], inputs
        nodes.append(node("Concat", parts, ["features"], [attr_i("axis", 1)], name="join"))
        return nodes, inits, "features", [batch, sum(dims) + m], inputs
    d = dims[0]
    if spelling == "b":
        inits.append(tensor("table", spec["shared"]))
        i64("offsets", spec["offsets"].reshape((1, k) if offsets_rank == 2 else (k,)))
        nodes.append(node("Add", ["x_cat", "offsets"], ["idx"], name="offset"))
        nodes.append(node("Gather", ["table", "idx"], ["tokens"], name="emb"))
    else:
        inits.append(tensor("table", spec["tables"][0]))
        nodes.append(node("Gather", ["table", "x_cat"], ["tokens"], name="emb"))
    if flatten == "window" or spelling == "c":
        return nodes, inits, "tokens", [batch, k, d], inputs
    if flatten == "flatten":
        nodes.append(node("Flatten", ["tokens"], ["flat"], [attr_i("axis", 1)], name="flatten"))
    else:
        i64("flat_shape", [-1, k * d])
        nodes.append(node("Reshape", ["tokens", "flat_shape"], ["flat"], name="flatten"))
    if not m:
        return nodes, inits, "flat", [batch, k * d], inputs
    nodes.append(node("Concat", ["flat", "x_num"], ["features"], [attr_i("axis", 1)], name="join"))
    return nodes, inits, "features", [batch, k * d + m], inputs


def embedding_from_spec(spec: dict, spelling: str = "a", tail: str = "mlp", encoder: dict | None = None, heads: Sequence[str] = ("mean",), **front) -> bytes:
    """The ONNX model of an embedding_spec() in one of EMBED_SPELLINGS (embedding_nodes; **front: its options).
    tail: "mlp" (the spec's Linear layers, MatMul + Add with Relu between; output 'Y'), "none" (the front end's result is the output 'Y'),
    "encoder": a transformer_spec() / from_torch_encoder() dict `encoder` with T = k and F = E = d behind the window (its positional constant,
    layers and head; outputs as transformer_from_spec names them)."""
    nodes, inits, cur, dims, inputs = embedding_nodes(spec, spelling, **front)
    if tail == "encoder":
        return transformer_from_spec(encoder, flat=False, heads=heads, front=(nodes, inits, cur, inputs))
    if tail == "mlp":
        for i, (W, b) in enumerate(spec["mlp"]):
            inits += [tensor(f"W{i}", W), tensor(f"B{i}", b)]
            nodes += [node("MatMul", [cur, f"W{i}"], [f"Z{i}"], name=f"fc{i}"), node("Add", [f"Z{i}", f"B{i}"], [f"H{i}"], name=f"fc{i}_bias")]
            cur = f"H{i}"
            if i + 1 < len(spec["mlp"]):
                nodes.append(node(spec["act"], [cur], [f"A{i}"], name=f"act{i}"))
                cur = f"A{i}"
        if spec["mlp"]:
            dims = dims[:-1] + [int(spec["mlp"][-1][0].shape[1])]
    nodes.append(node("Identity", [cur], ["Y"]))
    return model("embedding_" + spelling, nodes, inits, inputs, [value_info("Y", dims)], opset=13)


def embedding_lookup_reference(table, idx, offset=0) -> np.ndarray:
    """table[i] for i = trunc(idx) + offset with ONNX's negative indices (i in [-V, -1] counts from the end); raises IndexError beyond that."""
    t = np.asarray(table)
    i = np.trunc(np.asarray(idx, dtype=np.float64))
    if not np.all(np.isfinite(i)):
        raise IndexError("an index is not finite")
    i = i.astype(np.int64) + np.asarray(offset, dtype=np.int64)
    if np.any(i < -len(t)) or np.any(i >= len(t)):
        raise IndexError("an index is out of range")
    return t[np.where(i < 0, i + len(t), i)]


def embedding_reference(spec: dict, x_cat, x_num=None, spelling: str = "a", tail: str = "mlp", flatten: str = "reshape", encoder: dict | None = None,
                        heads: Sequence[str] = ("mean",)) -> dict:
    """numpy restatement of embedding_from_spec: {"features": the front end's result (f32, exact copies: table[idx], concatenation),
    "output": what follows it in float64 (the MLP, or the encoder's outputs as transformer_reference names them)}.  x_cat [N, k] index values
    (any real dtype: truncated toward zero), x_num [N, m] f32 or None."""
    x_cat = np.asarray(x_cat)
    k = len(spec["cards"])
    if spelling in ("a", "d"):
        parts = [embedding_lookup_reference(spec["tables"][j], x_cat[:, j]).reshape(len(x_cat), -1) for j in range(k)]
        feats = np.concatenate(parts + ([np.asarray(x_num, np.float32)] if spec["numeric"] else []), axis=1)
    else:
        tok = embedding_lookup_reference(spec["shared"], x_cat, spec["offsets"]) if spelling == "b" else embedding_lookup_reference(spec["tables"][0], x_cat)
        if spelling == "c" or flatten == "window":
            feats = tok
        else:
            feats = tok.reshape(len(tok), -1)
            if spec["numeric"]:
                feats = np.concatenate([feats, np.asarray(x_num, np.float32)], axis=1)
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    out = {"features": feats}
    if tail == "encoder":
        out["output"] = transformer_reference(encoder, feats, heads)
    elif tail == "mlp":
        h = feats.astype(np.float64)
        for i, (W, b) in enumerate(spec["mlp"]):
            h = h @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
            if i + 1 < len(spec["mlp"]):
                h = np.maximum(h, 0.0)
        out["output"] = h
    else:
        out["output"] = feats.astype(np.float64)
    return out


def embedding_inputs(spec: dict, rows: int, seed: int = 0, spelling: str = "a"):
    """Valid inputs of an embedding_spec(): (x_cat [rows, k] int64 with every column inside its table, x_num [rows, m] f32, and the one
    f32 table [rows, k + m] a call passes: x_cat's values beside x_num in input order).  Spelling (c): every column indexes table 0."""
    rng = np.random.default_rng(seed)
    cards = [spec["cards"][0]] * len(spec["cards"]) if spelling == "c" else spec["cards"]
    x_cat = np.stack([rng.integers(0, v, rows) for v in cards], axis=1).astype(np.int64)
    x_num = rng.standard_normal((rows, spec["numeric"])).astype(np.float32)
    m = 0 if spelling == "c" else spec["numeric"]
    return x_cat, x_num, np.ascontiguousarray(np.concatenate([x_cat.astype(np.float32), x_num[:, :m]], axis=1))


# ------------------------------------------------------------------------------------------
# Text encoders over padded token sequences (Embed window, per-row key masks, masked mean)
# ------------------------------------------------------------------------------------------

def text_encoder_spec(T: int = 16, V: int = 50, E: int = 32, h: int = 4, ff: int = 64, layers: int = 2, outputs: int = 3, pad_id: int = 0,
                      weight_scale: float = 1.0, seed: int = 91) -> dict:
    """Seeded BERT-shaped encoder: a token table [V, E] (N(0, 1) like nn.Embedding), a position table [T, E], LayerNorm, `layers` post-norm
    encoder layers (transformer_spec: its 'enc' entry, without input projection and positional constant of its own) and one Linear
    E -> outputs behind each head."""
    rng = np.random.default_rng(seed)
    enc = transformer_spec(T=T, F=E, E=E, h=h, ff=ff, layers=layers, norm_first=False, outputs=outputs, weight_scale=weight_scale, seed=seed + 1)
    enc["Win"] = enc["bin"] = enc["pos"] = None
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    return {"T": T, "V": V, "E": E, "pad_id": int(pad_id), "table": f32(rng.standard_normal((V, E))), "pos": f32(0.5 * rng.standard_normal((T, E))),
            "emb_ln": (f32(1.0 + 0.1 * rng.standard_normal(E)), f32(0.1 * rng.standard_normal(E))), "enc": enc}


def text_encoder_from_spec(spec: dict, form: str = "add", fill: float = float(np.finfo(np.float32).min), from_ids: bool = False,
                           heads: Sequence[str] = ("first", "masked_mean"), int_type: int = INT64, **mask_kw) -> bytes:
    """The ONNX model of a text_encoder_spec(): int64 input_ids [N, T] and, unless from_ids, attention_mask [N, T] (a call's columns in that
    order) -> Gather(table, ids) (node 'emb') -> Add(position table [T, E]) -> LayerNorm -> the encoder layers, every attention under the
    row mask (form, fill, from_ids: the mask is ids != pad_id written in the graph; **mask_kw: unsqueeze, expand) -> heads "first" (output
    'first') and "masked_mean" (output 'sentence'), each through the head Linear."""
    T, E = spec["T"], spec["E"]
    nodes = [node("Gather", ["table", "input_ids"], ["tokens"], name="emb"), node("Add", ["tokens", "pos_table"], ["tok_pos"], name="pos_add")]
    inits = [tensor("table", spec["table"]), tensor("pos_table", spec["pos"])]
    x = layernorm_nodes(nodes, inits, "tok_pos", spec["emb_ln"][0], spec["emb_ln"][1], "emb_norm", "emb_ln", spec["enc"]["eps"])
    inputs = [value_info("input_ids", ["N", T], int_type)] + ([] if from_ids else [value_info("attention_mask", ["N", T], int_type)])
    src = "input_ids" if from_ids else "attention_mask"
    pad = spec["pad_id"] if from_ids else None
    rm = dict(src=src, form=form, fill=fill, from_ids=pad, **mask_kw)
    return transformer_from_spec(spec["enc"], flat=False, heads=heads, front=(nodes, inits, x, inputs), row_mask=rm,
                                 mean_mask=dict(src=src, from_ids=pad))


def text_encoder_reference(spec: dict, ids, keep, form: str = "add", fill: float = float(np.finfo(np.float32).min),
                           heads: Sequence[str] = ("first", "masked_mean"), dtype=np.float64) -> dict:
    """numpy restatement of text_encoder_from_spec in `dtype` (float64: the reference; float32: what that format itself costs): ids [N, T]
    integers, keep [N, T] bool -> {output name: array}."""
    from math import erf
    enc, T, E = spec["enc"], spec["T"], spec["E"]
    fx = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    keep = np.asarray(keep, dtype=bool)
    ln = lambda a, g, b: fx(layernorm_reference(a, g, b, enc["eps"])) if dtype == np.float64 else _layernorm32(a, g, b, enc["eps"])  # noqa: E731
    x = ln(fx(spec["table"])[np.asarray(ids, dtype=np.int64)] + fx(spec["pos"]).reshape(1, T, E), spec["emb_ln"][0], spec["emb_ln"][1])
    act = (lambda a: np.maximum(a, 0)) if enc["act"] == "Relu" else (lambda a: fx(0.5 * a * (1.0 + np.vectorize(erf)(a / math.sqrt(2.0)))))
    for L in enc["layers"]:
        q, k, v = (x @ fx(L["W" + c]) + fx(L["b" + c]) for c in "qkv")
        a = masked_attention_reference(q, k, v, enc["h"], keep, fill, form, dtype=dtype)
        x = ln(x + (a @ fx(L["Wo"]) + fx(L["bo"])), L["g1"], L["be1"])
        x = ln(x + (act(x @ fx(L["W1"]) + fx(L["b1"])) @ fx(L["W2"]) + fx(L["b2"])), L["g2"], L["be2"])
    out = {}
    for hd in heads:
        v = x[:, 0] if hd == "first" else fx(masked_mean_reference(x, keep)) if dtype == np.float64 else _masked_mean32(x, keep)
        out["first" if hd == "first" else "sentence"] = v @ fx(enc["head_W"]) + fx(enc["head_b"])
    return out


def _layernorm32(x, g, b, eps):
    x = np.asarray(x, np.float32)
    n = np.float32(x.shape[-1])
    d = x - x.sum(axis=-1, keepdims=True, dtype=np.float32) / n
    var = (d * d).sum(axis=-1, keepdims=True, dtype=np.float32) / n
    return d / np.sqrt(var + np.float32(eps)) * np.asarray(g, np.float32) + np.asarray(b, np.float32)


def _masked_mean32(x, keep, clip: float = 1e-9):
    s = np.where(keep[:, :, None], np.asarray(x, np.float32), np.float32(0)).sum(axis=1, dtype=np.float32)
    return s / np.maximum(keep.sum(axis=1, keepdims=True).astype(np.float32), np.float32(clip))


def text_encoder_inputs(spec: dict, lengths, seed: int = 0, left: bool = False):
    """(ids [N, T] int64 with pad_id outside each row's length and never inside it, keep [N, T] bool, the f32 table of a call with a mask
    input [N, 2T]: ids beside the 0 / 1 mask, the one of a from_ids model [N, T]); left: padded on the left."""
    T, V, pad = spec["T"], spec["V"], spec["pad_id"]
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    pos = np.arange(T)[None, :]
    keep = pos >= (T - lengths)[:, None] if left else pos < lengths[:, None]
    ids = rng.integers(0, V - 1, (len(lengths), T))
    ids = np.where(ids >= pad, ids + 1, ids)  # (every value but pad_id)
    ids = np.where(keep, ids, pad).astype(np.int64)
    both = np.ascontiguousarray(np.concatenate([ids, keep.astype(np.int64)], axis=1).astype(np.float32))
    return ids, keep, both, np.ascontiguousarray(ids.astype(np.float32))


# ------------------------------------------------------------------------------------------
# Feature interactions of recommender models (DLRM's pairwise dots, the FM / DeepFM / NFM bi-interaction term)
# ------------------------------------------------------------------------------------------
INTERACT_SOURCES = ("input", "embed", "reshape", "concat")


def interact_window_nodes(k: int, d: int, source: str = "reshape", table=None, batch: int | str = "N"):
    """A window T [N, k, d] as (nodes, initializers, its name 'T', graph inputs, width of the f32 table a call passes).
    "input": the graph input X [N, k, d] itself.  "reshape": Reshape of the input X [N, k * d] (DLRM's .view(N, -1, d)).  "concat": the k
    column blocks of X [N, k * d], each Slice -> Unsqueeze(1) -> [N, 1, d], joined by Concat(axis = 1).  "embed": Gather(table [V, d],
    x_cat [N, k] int64), an Embed window; the call passes the k index values."""
    assert source in INTERACT_SOURCES
    nodes, inits = [], []
    i64 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.int64)))  # noqa: E731
    if source == "input":
        nodes.append(node("Identity", ["X"], ["T"], name="window"))
        return nodes, inits, "T", [value_info("X", [batch, k, d])], k * d
    if source == "embed":
        assert table is not None and table.shape[1] == d
        inits.append(tensor("table", np.asarray(table, np.float32)))
        nodes.append(node("Gather", ["table", "x_cat"], ["T"], name="emb"))
        return nodes, inits, "T", [value_info("x_cat", [batch, k], INT64)], k
    inputs = [value_info("X", [batch, k * d])]
    if source == "reshape":
        i64("window_shape", [-1, k, d])
        nodes.append(node("Reshape", ["X", "window_shape"], ["T"], name="window"))
        return nodes, inits, "T", inputs, k * d
    i64("ax1", [1])
    for j in range(k):
        i64(f"b{j}", [j * d]); i64(f"e{j}", [(j + 1) * d])  # noqa: E702
        nodes.append(node("Slice", ["X", f"b{j}", f"e{j}", "ax1"], [f"f{j}"], name=f"field{j}"))
        nodes.append(node("Unsqueeze", [f"f{j}", "ax1"], [f"u{j}"], name=f"unsq{j}"))
    nodes.append(node("Concat", [f"u{j}" for j in range(k)], ["T"], [attr_i("axis", 1)], name="stack"))
    return nodes, inits, "T", inputs, k * d


def interact_dot_nodes(nodes: list, inits: list, T: str, k: int, form: str = "gather", sel=None, flatten: str = "flatten", perm=(0, 2, 1),
                       right: str | None = None) -> tuple[str, list]:
    """Appends Z = MatMul(T, Transpose(T, perm)) (nodes 'tr', 'dot') and what reads it; returns (result name, its dims behind the row axis).
    form "matrix": Z [N, k, k] itself; "flat": Flatten / Reshape (`flatten`) to [N, k * k]; "gather": that, then Gather(axis = 1) by the
    constant list `sel` (node 'pairs'); "index" / "index_folded": the TorchScript exporter's Z[:, li, lj] (_advanced_index_nodes).
    right: the value the Transpose reads (default T: a Gram matrix)."""
    nodes.append(node("Transpose", [right or T], ["Tt"], [attr_ints("perm", perm)], name="tr"))
    nodes.append(node("MatMul", [T, "Tt"], ["Z"], name="dot"))
    if form == "matrix":
        return "Z", [k, k]
    if form in ("index", "index_folded"):
        return _advanced_index_nodes(nodes, inits, k, np.asarray(sel, dtype=np.int64).reshape(-1), form == "index_folded")
    if flatten == "flatten":
        nodes.append(node("Flatten", ["Z"], ["Zflat"], [attr_i("axis", 1)], name="zflat"))
    else:
        inits.append(tensor("zflat_shape", np.asarray([-1, k * k], dtype=np.int64)))
        nodes.append(node("Reshape", ["Z", "zflat_shape"], ["Zflat"], name="zflat"))
    if form == "flat":
        return "Zflat", [k * k]
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    inits.append(tensor("pairs_i", sel))
    nodes.append(node("Gather", ["Zflat", "pairs_i"], ["Zsel"], [attr_i("axis", 1)], name="pairs"))
    return "Zsel", [len(sel)]


def _advanced_index_nodes(nodes: list, inits: list, k: int, sel: np.ndarray, folded: bool) -> tuple[str, list]:
    """Z[:, li, lj] as the TorchScript exporter writes it, node for node as torch/onnx/symbolic_opset9.py::index builds it for two index
    tensors on axes 1 and 2 of a rank-3 value (read from that source, not exported): the three dims by Shape -> Gather, Transpose(1,2,0),
    Flatten(2), the index lj + li * dim2 by Mul and Add, Gather(axis = 0), Reshape to [-1, dim0], Transpose(1,0), Reshape to
    Concat(dim0, Shape(index)).  li, lj = divmod(sel, k), so sel must be non-negative.  folded: what constant folding leaves where the dims
    are static -- the index one constant, the Reshape targets [P, -1] and [-1, P]."""
    assert np.all(sel >= 0)
    i64 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.int64)))  # noqa: E731
    P = len(sel)
    nodes.append(node("Transpose", ["Z"], ["Zt"], [attr_ints("perm", [1, 2, 0])], name="idx_front"))
    nodes.append(node("Flatten", ["Zt"], ["Zf"], [attr_i("axis", 2)], name="idx_flat"))
    if folded:
        i64("cum", sel); i64("fold_shape", [P, -1]); i64("final_shape", [-1, P])  # noqa: E702
    else:
        i64("li", sel // k); i64("lj", sel % k); i64("minus1", [-1])  # noqa: E702
        nodes.append(node("Shape", ["Z"], ["zshape"], name="zshape"))
        for a in range(3):
            i64(f"dim{a}_i", [a])
            nodes.append(node("Gather", ["zshape", f"dim{a}_i"], [f"dim{a}"], [attr_i("axis", 0)], name=f"dim{a}"))
        nodes.append(node("Mul", ["li", "dim2"], ["li_scaled"], name="idx_mul"))
        nodes.append(node("Add", ["lj", "li_scaled"], ["cum"], name="idx_add"))
    nodes.append(node("Gather", ["Zf", "cum"], ["Zg"], [attr_i("axis", 0)], name="pairs"))
    if not folded:
        nodes.append(node("Shape", ["cum"], ["cum_shape"], name="cum_shape"))
        nodes.append(node("Concat", ["minus1", "dim0"], ["fold_shape"], [attr_i("axis", 0)], name="fold_shape"))
        nodes.append(node("Concat", ["dim0", "cum_shape"], ["final_shape"], [attr_i("axis", 0)], name="final_shape"))
    nodes.append(node("Reshape", ["Zg", "fold_shape"], ["Zr"], name="idx_fold"))
    nodes.append(node("Transpose", ["Zr"], ["Zb"], [attr_ints("perm", [1, 0])], name="idx_back"))
    nodes.append(node("Reshape", ["Zb", "final_shape"], ["Zsel"], name="idx_final"))
    return "Zsel", [P]


def interact_triangle(k: int, diagonal: bool = False) -> np.ndarray:
    """li * k + lj over the lower triangle (i > j; diagonal: i >= j), row by row: DLRM's Z[:, li, lj]."""
    return np.asarray([i * k + j for i in range(k) for j in range(i + 1 if diagonal else i)], dtype=np.int64)


def interact_dot_model(k: int, d: int, form: str = "gather", sel=None, source: str = "reshape", table=None, batch: int | str = "N", **kw) -> bytes:
    nodes, inits, T, inputs, _ = interact_window_nodes(k, d, source, table, batch)
    cur, dims = interact_dot_nodes(nodes, inits, T, k, form, sel, **kw)
    nodes.append(node("Identity", [cur], ["Y"]))
    return model("interact_dot", nodes, inits, inputs, [value_info("Y", [batch] + dims)], opset=13)


def interact_fm_nodes(nodes: list, inits: list, T: str, d: int, square: str = "mul", h=None, h_side: str = "right", sum_last: bool = False,
                      keepdims: int = 0, last_keepdims: int = 1, h_after: bool = False, axes_input: bool = True) -> tuple[str, list]:
    """Appends the bi-interaction term of T [N, k, d] as written: S = ReduceSum(T, [1]) ('fsum'), S * S or S ^ 2 ('sq_sum'), T * T or T ^ 2
    ('sq'), its ReduceSum ('sum_sq'), Sub ('diff'), then Mul by the constant scalar h on h_side ('half') and, with sum_last, ReduceSum over
    the last axis ('total'); h_after: the Mul follows that sum.  Returns (result name, its dims behind the row axis)."""
    def rsum(x, y, axes, keep, name):
        if axes_input:
            inits.append(tensor(name + "_axes", np.asarray(axes, dtype=np.int64)))
            nodes.append(node("ReduceSum", [x, name + "_axes"], [y], [attr_i("keepdims", keep)], name=name))
        else:
            nodes.append(node("ReduceSum", [x], [y], [attr_ints("axes", axes), attr_i("keepdims", keep)], name=name))

    def sq(x, y, name):
        if square == "mul":
            nodes.append(node("Mul", [x, x], [y], name=name))
        else:
            if not any(b"two" in t[:8] for t in inits):
                inits.append(tensor("two", np.asarray(2.0, dtype=np.float32)))
            nodes.append(node("Pow", [x, "two"], [y], name=name))

    rsum(T, "S", [1], keepdims, "fsum")
    sq("S", "SS", "sq_sum")
    sq(T, "Q", "sq")
    rsum("Q", "QS", [1], keepdims, "sum_sq")
    nodes.append(node("Sub", ["SS", "QS"], ["D"], name="diff"))
    cur, dims = "D", ([1, d] if keepdims else [d])

    def mul_h(cur):
        inits.append(tensor("h", np.asarray(h, dtype=np.float32)))
        nodes.append(node("Mul", [cur, "h"] if h_side == "right" else ["h", cur], ["Dh"], name="half"))
        return "Dh"

    if h is not None and not h_after:
        cur = mul_h(cur)
    if sum_last:
        rsum(cur, "Dsum", [-1], last_keepdims, "total")
        cur, dims = "Dsum", (dims[:-1] + [1] if last_keepdims else dims[:-1])
    if h is not None and h_after:
        cur = mul_h(cur)
    return cur, dims


def interact_fm_model(k: int, d: int, source: str = "reshape", table=None, batch: int | str = "N", opset: int = 13, **kw) -> bytes:
    nodes, inits, T, inputs, _ = interact_window_nodes(k, d, source, table, batch)
    cur, dims = interact_fm_nodes(nodes, inits, T, d, **kw)
    nodes.append(node("Identity", [cur], ["Y"]))
    return model("interact_fm", nodes, inits, inputs, [value_info("Y", [batch] + dims)], opset=opset)


def interact_dot_reference(T, sel=None) -> np.ndarray:
    """float64: Z = T T^T per row, [N, k, k]; with sel, Z.reshape(N, k * k)[:, sel] (negative indices count from the end)."""
    t = np.asarray(T, np.float64)
    z = np.einsum("nic,njc->nij", t, t)
    return z if sel is None else z.reshape(len(t), -1)[:, np.asarray(sel, dtype=np.int64)]


def interact_fm_reference(T, h=None, sum_last: bool = False) -> np.ndarray:
    """float64: h * ((sum_f T)^2 - sum_f T^2), [N, d]; sum_last: its sum over the last axis, [N, 1]."""
    t = np.asarray(T, np.float64)
    v = t.sum(axis=1) ** 2 - (t * t).sum(axis=1)
    if h is not None:
        v = v * float(h)
    return v.sum(axis=1, keepdims=True) if sum_last else v


def _mlp_layers(rng, widths, scale):
    out = []
    for i, o in zip(widths[:-1], widths[1:]):
        b = scale / np.sqrt(i)
        out.append((rng.uniform(-b, b, (i, o)).astype(np.float32), rng.uniform(-b, b, (o,)).astype(np.float32)))
    return out


def _mlp_nodes(nodes, inits, cur, layers, p, last_act):
    for i, (W, b) in enumerate(layers):
        inits += [tensor(f"{p}W{i}", W), tensor(f"{p}B{i}", b)]
        nodes += [node("MatMul", [cur, f"{p}W{i}"], [f"{p}Z{i}"], name=f"{p}fc{i}"), node("Add", [f"{p}Z{i}", f"{p}B{i}"], [f"{p}H{i}"], name=f"{p}fc{i}_bias")]
        cur = f"{p}H{i}"
        if i + 1 < len(layers) or last_act:
            nodes.append(node("Relu", [cur], [f"{p}A{i}"], name=f"{p}act{i}"))
            cur = f"{p}A{i}"
    return cur


def _mlp64(h, layers, last_act):
    for i, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
        if i + 1 < len(layers) or last_act:
            h = np.maximum(h, 0.0)
    return h


def dlrm_spec(cards: Sequence[int] = (7, 11, 5), d: int = 4, numeric: int = 3, bottom: Sequence[int] = (8,), top: Sequence[int] = (8,), seed: int = 81,
              weight_scale: float = 1.0, diagonal: bool = False) -> dict:
    """Seeded DLRM: `numeric` dense columns -> bottom MLP (... -> d, Relu after every layer) = x; one table [cards[j], d] per categorical
    column; T = cat([x] + lookups, 1).view(N, -1, d); Z = bmm(T, T^T); R = cat([x, Z.flatten(1)[:, li * K + lj]], 1) over the strict lower
    triangle (diagonal: with it); top MLP R -> ... -> 1 (Relu between the layers).  Weights U(+-weight_scale / sqrt(fan_in))."""
    rng = np.random.default_rng(seed)
    K = len(cards) + 1
    sel = interact_triangle(K, diagonal)
    return {"cards": [int(v) for v in cards], "d": int(d), "numeric": int(numeric), "sel": sel,
            "tables": [rng.standard_normal((int(v), d)).astype(np.float32) for v in cards],
            "bottom": _mlp_layers(rng, [numeric] + list(bottom) + [d], weight_scale), "top": _mlp_layers(rng, [d + len(sel)] + list(top) + [1], weight_scale)}


def from_torch_dlrm(embeddings, bottom, top, diagonal: bool = False) -> dict:
    """The dlrm_spec() dict of torch modules: nn.Embedding tables, the nn.Linear layers of the bottom and of the top MLP, in order."""
    lin = lambda m: (m.weight.detach().cpu().numpy().astype(np.float32).T.copy(), m.bias.detach().cpu().numpy().astype(np.float32).copy())  # noqa: E731
    tables = [e.weight.detach().cpu().numpy().astype(np.float32).copy() for e in embeddings]
    return {"cards": [int(t.shape[0]) for t in tables], "d": int(tables[0].shape[1]), "numeric": int(bottom[0].in_features), "tables": tables,
            "sel": interact_triangle(len(tables) + 1, diagonal), "bottom": [lin(m) for m in bottom], "top": [lin(m) for m in top]}


def dlrm_from_spec(spec: dict, batch: int | str = "N", extra_outputs: bool = False, form: str = "gather") -> bytes:
    """Inputs x_cat [N, k] int64 and x_num [N, m] (a call passes the k index values beside the m dense columns).  Output 'Y' [N, 1];
    extra_outputs: also 'R' (the top MLP's input: x beside the chosen products) and 'xb' (the bottom MLP's result)."""
    k, d, m = len(spec["cards"]), spec["d"], spec["numeric"]
    nodes, inits = [], []
    inputs = [value_info("x_cat", [batch, k], INT64), value_info("x_num", [batch, m])]
    x = _mlp_nodes(nodes, inits, "x_num", spec["bottom"], "bot_", True)
    parts = [x]
    for j in range(k):
        inits += [tensor(f"col{j}_i", np.asarray(j, dtype=np.int64)), tensor(f"table{j}", spec["tables"][j])]
        nodes.append(node("Gather", ["x_cat", f"col{j}_i"], [f"col{j}"], [attr_i("axis", 1)], name=f"pick{j}"))
        nodes.append(node("Gather", [f"table{j}", f"col{j}"], [f"e{j}"], name=f"emb{j}"))
        parts.append(f"e{j}")
    nodes.append(node("Concat", parts, ["features"], [attr_i("axis", 1)], name="join"))
    inits.append(tensor("window_shape", np.asarray([-1, k + 1, d], dtype=np.int64)))
    nodes.append(node("Reshape", ["features", "window_shape"], ["T"], name="window"))
    zsel, _ = interact_dot_nodes(nodes, inits, "T", k + 1, form, spec["sel"])
    nodes.append(node("Concat", [x, zsel], ["R"], [attr_i("axis", 1)], name="cat_r"))
    y = _mlp_nodes(nodes, inits, "R", spec["top"], "top_", False)
    nodes.append(node("Identity", [y], ["Y"]))
    outputs = [value_info("Y", [batch, 1])]
    if extra_outputs:
        nodes.append(node("Identity", [x], ["xb"]))
        outputs += [value_info("R", [batch, d + len(spec["sel"])]), value_info("xb", [batch, d])]
    return model("dlrm", nodes, inits, inputs, outputs, opset=13)


def dlrm_reference(spec: dict, x_cat, x_num) -> dict:
    """float64 restatement of dlrm_from_spec: {"x": the bottom MLP's result, "T", "R", "output"}."""
    x = _mlp64(np.asarray(x_num, np.float64), spec["bottom"], True)
    T = np.stack([x] + [np.asarray(t, np.float64)[np.asarray(x_cat)[:, j]] for j, t in enumerate(spec["tables"])], axis=1)
    R = np.concatenate([x, interact_dot_reference(T, spec["sel"])], axis=1)
    return {"x": x, "T": T, "R": R, "output": _mlp64(R, spec["top"], False)}


def deepfm_spec(cards: Sequence[int] = (7, 11, 5, 3), d: int = 4, hidden: Sequence[int] = (8,), seed: int = 83, weight_scale: float = 1.0) -> dict:
    """Seeded DeepFM over len(cards) categorical fields: one shared table [sum(cards), d] and a first-order table [sum(cards), 1] indexed by
    x_cat + offsets; y = sum_f w[f] + 0.5 * sum_c((sum_f v)^2 - sum_f v^2) + MLP(flatten(v))."""
    rng = np.random.default_rng(seed)
    V, k = int(sum(cards)), len(cards)
    return {"cards": [int(v) for v in cards], "d": int(d), "table": rng.standard_normal((V, d)).astype(np.float32),
            "first": (rng.standard_normal((V, 1)) * weight_scale).astype(np.float32),
            "offsets": np.concatenate([[0], np.cumsum(cards)[:-1]]).astype(np.int64), "mlp": _mlp_layers(rng, [k * d] + list(hidden) + [1], weight_scale)}


def deepfm_from_spec(spec: dict, batch: int | str = "N") -> bytes:
    """Input x_cat [N, k] int64; output 'Y' [N, 1] = first-order sum + FM second-order term + deep MLP."""
    k, d = len(spec["cards"]), spec["d"]
    nodes, inits = [], []
    inits += [tensor("offsets", spec["offsets"]), tensor("table", spec["table"]), tensor("first", spec["first"])]
    nodes.append(node("Add", ["x_cat", "offsets"], ["idx"], name="offset"))
    nodes.append(node("Gather", ["table", "idx"], ["T"], name="emb"))
    nodes.append(node("Gather", ["first", "idx"], ["w"], name="emb_first"))
    nodes.append(node("Flatten", ["w"], ["wflat"], [attr_i("axis", 1)], name="first_flat"))
    inits.append(tensor("last_axis", np.asarray([-1], dtype=np.int64)))
    nodes.append(node("ReduceSum", ["wflat", "last_axis"], ["y1"], [attr_i("keepdims", 1)], name="first_sum"))
    y2, _ = interact_fm_nodes(nodes, inits, "T", d, square="mul", h=0.5, sum_last=True, keepdims=0, last_keepdims=1, h_after=True)
    nodes.append(node("Flatten", ["T"], ["deep_in"], [attr_i("axis", 1)], name="deep_flat"))
    y3 = _mlp_nodes(nodes, inits, "deep_in", spec["mlp"], "deep_", False)
    nodes.append(node("Add", ["y1", y2], ["y12"], name="add_fm"))
    nodes.append(node("Add", ["y12", y3], ["Y"], name="add_deep"))
    return model("deepfm", nodes, inits, [value_info("x_cat", [batch, k], INT64)], [value_info("Y", [batch, 1])], opset=13)


def deepfm_reference(spec: dict, x_cat) -> dict:
    """float64 restatement of deepfm_from_spec: {"T", "fm", "output"}."""
    idx = np.asarray(x_cat, dtype=np.int64) + spec["offsets"]
    T = np.asarray(spec["table"], np.float64)[idx]
    y1 = np.asarray(spec["first"], np.float64)[idx][:, :, 0].sum(axis=1, keepdims=True)
    fm = interact_fm_reference(T, None, True) * 0.5
    return {"T": T, "fm": fm, "output": y1 + fm + _mlp64(T.reshape(len(T), -1), spec["mlp"], False)}


# ------------------------------------------------------------------------------------------
# The opset-23 operators Attention and RMSNormalization, and a pre-norm decoder block over them
# ------------------------------------------------------------------------------------------

def attention_op_nodes(nodes: list, inits: list, p: str, q: str, k: str, v: str, Tq: int, Tk: int, hq: int, hkv: int, dh: int, form: str = "4d",
                       causal: bool = False, mask=None, mask_value: str | None = None, scale: float | None = None, extra_attrs: Sequence[bytes] = (),
                       extra_inputs: Sequence[str] = (), extra_outputs: Sequence[str] = (), rotary=None) -> str:
    """Appends one standard-domain Attention node '<p>attn' over q [N, Tq, hq dh], k, v [N, Tk, hkv dh] (names) and returns the name of its
    [N, Tq, hq dh] result.  form "3d": the operands as they are, beside q_num_heads / kv_num_heads; "4d" (what torch's exporter writes): each
    through Reshape [0, T, h, dh] -> Transpose(0,2,1,3), and Y back through Transpose(0,2,1,3) -> Reshape [0, Tq, hq dh].
    mask: a constant attn_mask (float32 additive or bool, true = kept); mask_value: the name of a value computed in the graph instead;
    scale: the attribute (None: left out, the operator's 1 / sqrt(dh)); extra_inputs follow attn_mask (past_key, past_value,
    nonpad_kv_seqlen; "" = absent), extra_outputs follow Y.
    rotary: None, True or the options of rotary_options(): a rotary embedding on the operands named in its "on" ("qk"), head-major behind the
    head split (form "4d") or as the 3-D operator beside num_heads in front of the node (form "3d": the operator form only)."""
    i64 = lambda name, val: inits.append(tensor(name, np.asarray(val, dtype=np.int64)))  # noqa: E731
    rot = rotary_options(rotary)
    attrs = [attr_i("is_causal", 1)] if causal else []
    if scale is not None:
        attrs.append(attr_f("scale", scale))
    ops = [q, k, v]
    if form == "4d":
        for j, (nm, T, h) in enumerate((("q", Tq, hq), ("k", Tk, hkv), ("v", Tk, hkv))):
            i64(p + nm + "_split", [0, T, h, dh])
            nodes += [node("Reshape", [ops[j], p + nm + "_split"], [p + nm + "4"], name=p + "split_" + nm),
                      node("Transpose", [p + nm + "4"], [p + nm + "h"], [attr_ints("perm", [0, 2, 1, 3])], name=p + "tr_" + nm)]
            ops[j] = p + nm + "h"
            if rot is not None and nm in rot["on"]:
                ops[j] = rotary_nodes(nodes, inits, p + nm + "_", ops[j], T, dh, rot)
    else:
        attrs += [attr_i("q_num_heads", hq), attr_i("kv_num_heads", hkv)]
        for j, (nm, T, h) in enumerate((("q", Tq, hq), ("k", Tk, hkv), ("v", Tk, hkv))):
            if rot is not None and nm in rot["on"]:
                ops[j] = rotary_nodes(nodes, inits, p + nm + "_", ops[j], T, dh, rot, num_heads=h)
    if mask is not None:
        inits.append(tensor(p + "mask", np.asarray(mask)))
        mask_value = p + "mask"
    ins = ops + ([mask_value] if mask_value is not None else [""] if extra_inputs else []) + list(extra_inputs)
    y = p + ("y4" if form == "4d" else "o")
    nodes.append(node("Attention", ins, [y] + list(extra_outputs), list(attrs) + list(extra_attrs), name=p + "attn"))
    if form == "4d":
        i64(p + "merge", [0, Tq, hq * dh])
        nodes += [node("Transpose", [y], [p + "ot"], [attr_ints("perm", [0, 2, 1, 3])], name=p + "tr_o"),
                  node("Reshape", [p + "ot", p + "merge"], [p + "o"], name=p + "merge_heads")]
    return p + "o"


def bool_row_mask_value(nodes: list, inits: list, p: str, T: int, src: str = "M", kind: str = "cast", pad: int = 0, lift: str = "unsqueeze") -> str:
    """Appends a per-row bool key mask [N, 1, 1, T], true = kept, from the [N, T] graph input src: kind "cast": Cast(to = BOOL) of HF's 0 / 1
    attention_mask; "ids": Not(Equal(ids, pad)); "equal": Equal(ids, pad) alone (true = MASKED: refused); "float": Cast(to = FLOAT) (refused).
    lift: "unsqueeze" (axes [1, 2]) or "reshape" ([-1, 1, 1, T])."""
    i64 = lambda name, val: inits.append(tensor(name, np.asarray(val, dtype=np.int64)))  # noqa: E731
    if kind in ("cast", "float"):
        nodes.append(node("Cast", [src], [p + "keep"], [attr_i("to", BOOL if kind == "cast" else FLOAT)], name=p + "cast"))
    else:
        i64(p + "pad", pad)
        nodes.append(node("Equal", [src, p + "pad"], [p + ("eq" if kind == "ids" else "keep")], name=p + "equal"))
        if kind == "ids":
            nodes.append(node("Not", [p + "eq"], [p + "keep"], name=p + "not"))
    if lift == "reshape":
        i64(p + "s4", [-1, 1, 1, T])
        nodes.append(node("Reshape", [p + "keep", p + "s4"], [p + "keep4"], name=p + "reshape"))
    else:
        i64(p + "a12", [1, 2])
        nodes.append(node("Unsqueeze", [p + "keep", p + "a12"], [p + "keep4"], name=p + "unsqueeze"))
    return p + "keep4"


def attention_op_model(Tq: int, Tk: int, hq: int, hkv: int, dh: int, form: str = "4d", causal: bool = False, mask=None, row_mask: dict | None = None,
                       scale: float | None = None, opset: int = 23, packed: bool = False, mask_type: int = INT64, **kw) -> bytes:
    """The Attention operator alone over flat inputs Q [N, Tq hq dh], K, V [N, Tk hkv dh] (the call's columns in that order), each reshaped to
    [N, T, E]; packed (Tq = Tk, hq = hkv): X [N, T 3E] -> Reshape -> Split on the last axis.  row_mask: the keyword arguments of
    bool_row_mask_value, for one more input M [N, Tk] (mask_type) behind the others.  Output [N, Tq, hq dh].  kw: attention_op_nodes (rotary =
    ... among them), and graph_outputs: names of further graph outputs."""
    nodes, inits = [], []
    Eq, Ekv = hq * dh, hkv * dh
    if packed:
        assert Tq == Tk and hq == hkv
        inits += [tensor("x_shape", np.asarray([-1, Tq, 3 * Eq], dtype=np.int64)), tensor("sp", np.asarray([Eq, Eq, Eq], dtype=np.int64))]
        nodes += [node("Reshape", ["X", "x_shape"], ["X3"]), node("Split", ["X3", "sp"], ["q", "k", "v"], [attr_i("axis", 2)], name="split_qkv")]
        ins = [value_info("X", ["N", Tq * 3 * Eq])]
    else:
        for nm, T, E in (("q", Tq, Eq), ("k", Tk, Ekv), ("v", Tk, Ekv)):
            inits.append(tensor(nm + "_shape", np.asarray([-1, T, E], dtype=np.int64)))
            nodes.append(node("Reshape", [nm.upper(), nm + "_shape"], [nm]))
        ins = [value_info("Q", ["N", Tq * Eq]), value_info("K", ["N", Tk * Ekv]), value_info("V", ["N", Tk * Ekv])]
    if row_mask is not None:
        ins.append(value_info("M", ["N", Tk], mask_type))
        kw["mask_value"] = bool_row_mask_value(nodes, inits, "rm_", Tk, **row_mask)
    more_outputs = [value_info(o, ["N"]) for o in kw.pop("graph_outputs", ())]  # further graph outputs (never served: the first one is)
    out = attention_op_nodes(nodes, inits, "a_", "q", "k", "v", Tq, Tk, hq, hkv, dh, form=form, causal=causal, mask=mask, scale=scale, **kw)
    return model("attention_op", nodes, inits, ins, [value_info(out, ["N", Tq, Eq])] + more_outputs, opset=opset)


def attention_op_reference(q, k, v, hq: int, hkv: int, scale: float | None = None, causal: bool = False, mask=None, keep=None) -> np.ndarray:
    """float64 numpy restatement of the operator over q [N, Tq, hq dh], k, v [N, Tk, hkv dh]: query head g reads K / V head g // (hq // hkv);
    causal: key j counts iff j <= i (top-left aligned); mask: additive [Tq, Tk] (broadcast) or bool, true = kept; keep: [N, Tk] bool per row."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    N, Tq, Eq = q.shape
    Tk, dh, g = k.shape[1], Eq // hq, hq // hkv
    sp = lambda a, T, h: a.reshape(N, T, h, dh).transpose(0, 2, 1, 3)  # noqa: E731
    kh, vh = (np.repeat(sp(a, Tk, hkv), g, axis=1) for a in (k, v))
    with np.errstate(all="ignore"):
        s = sp(q, Tq, hq) @ kh.transpose(0, 1, 3, 2) * ((1.0 / math.sqrt(dh)) if scale is None else float(np.float32(scale)))
        if mask is not None:
            mk = np.asarray(mask)
            mk = np.where(mk, 0.0, -np.inf) if mk.dtype == np.bool_ else mk.astype(np.float64)
            s = s + np.broadcast_to(mk.reshape(mk.shape[-2:]), (Tq, Tk))
        if causal:
            s = np.where(np.arange(Tk)[None, :] <= np.arange(Tq)[:, None], s, -np.inf)
        if keep is not None:
            s = np.where(np.asarray(keep, dtype=bool).reshape(N, 1, 1, Tk), s, -np.inf)
        s = s - s.max(axis=-1, keepdims=True)
        pr = np.exp(s)
        pr = pr / pr.sum(axis=-1, keepdims=True)
        return (pr @ vh).transpose(0, 2, 1, 3).reshape(N, Tq, Eq)


def rmsnorm_reference(x, g, eps: float) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + np.float64(np.float32(eps))) * np.asarray(g, dtype=np.float64)


def rmsnorm_model(E: int, eps: float, g, T: int = 0, axis: int = -1, opset: int = 23, extra_attrs: Sequence[bytes] = (), scale_input: bool = False) -> bytes:
    """RMSNormalization(axis -1) on [N, E] (T = 0) or on [N, T, E] behind a Reshape; node 'rms'.  scale_input: the scale is a second graph
    input (refused: only a constant)."""
    inits = [] if scale_input else [tensor("g", np.asarray(g, np.float32))]
    nodes = []
    if T:
        inits.append(tensor("s", np.asarray([-1, T, E], np.int64)))
        nodes.append(node("Reshape", ["X", "s"], ["x3"]))
    nodes.append(node("RMSNormalization", ["x3" if T else "X", "g"], ["out"], [attr_i("axis", axis), attr_f("epsilon", eps)] + list(extra_attrs), name="rms"))
    ins = [value_info("X", ["N", max(T, 1) * E])] + ([value_info("g", ["N", E])] if scale_input else [])
    return model("rms", nodes, inits, ins, [value_info("out", ["N", T, E] if T else ["N", E])], opset=opset)


def decoder_block_spec(T: int = 16, E: int = 32, hq: int = 4, hkv: int = 2, ff: int = 64, layers: int = 2, outputs: int = 3, eps: float = 1e-6,
                       weight_scale: float = 1.0, seed: int = 91, rotary=None) -> dict:
    """Seeded pre-norm Llama-style decoder blocks over a window [N, T, E]: RMSNorm -> Q (E -> E), K, V (E -> hkv dh) -> causal grouped attention ->
    projection -> residual -> RMSNorm -> SwiGLU (Swish(x Wg) * (x Wu)) Wd -> residual; a final RMSNorm and a Linear head on the last step.
    Matrices are [in, out], no biases but the head's.  rotary: None, True or the options of rotary_options(): Q and K of every layer are
    rotated (spec["rotary"]; absent when off)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    lin = lambda i, o: f32(rng.uniform(-1, 1, (i, o)) * weight_scale / np.sqrt(i))  # noqa: E731
    dh = E // hq
    ls = [{"Wq": lin(E, E), "Wk": lin(E, hkv * dh), "Wv": lin(E, hkv * dh), "Wo": lin(E, E), "Wg": lin(E, ff), "Wu": lin(E, ff), "Wd": lin(ff, E),
           "g1": f32(1.0 + 0.1 * rng.standard_normal(E)), "g2": f32(1.0 + 0.1 * rng.standard_normal(E))} for _ in range(layers)]
    spec = {"T": T, "E": E, "hq": hq, "hkv": hkv, "ff": ff, "eps": eps, "layers": ls, "g_final": f32(1.0 + 0.1 * rng.standard_normal(E)),
            "head_W": lin(E, outputs), "head_b": f32(rng.uniform(-1, 1, outputs) / np.sqrt(E))}
    if rotary_options(rotary) is not None:
        spec["rotary"] = rotary_options(rotary)
    return spec


def from_torch_decoder_block(blocks, final_norm, head, T: int, hq: int, hkv: int) -> dict:
    """The decoder_block_spec() dict of torch modules: each block has the bias-free Linears q_proj, k_proj, v_proj, o_proj, gate, up, down and the
    nn.RMSNorm modules norm1, norm2; final_norm an nn.RMSNorm, head an nn.Linear."""
    w = lambda lin: lin.weight.detach().cpu().numpy().astype(np.float32).T.copy()  # noqa: E731
    g = lambda nrm: nrm.weight.detach().cpu().numpy().astype(np.float32)  # noqa: E731
    ls = [{"Wq": w(b.q_proj), "Wk": w(b.k_proj), "Wv": w(b.v_proj), "Wo": w(b.o_proj), "Wg": w(b.gate), "Wu": w(b.up), "Wd": w(b.down), "g1": g(b.norm1),
           "g2": g(b.norm2)} for b in blocks]
    E = ls[0]["Wq"].shape[0]
    return {"T": T, "E": E, "hq": hq, "hkv": hkv, "ff": ls[0]["Wg"].shape[1], "eps": float(blocks[0].norm1.eps), "layers": ls, "g_final": g(final_norm),
            "head_W": w(head), "head_b": head.bias.detach().cpu().numpy().astype(np.float32)}


def decoder_block_from_spec(spec: dict, form: str = "4d", opset: int = 23, rotary=None) -> bytes:
    """The ONNX model of a decoder_block_spec(): X [N, T E] -> Reshape [N, T, E] -> the blocks -> the last step -> Linear: output "last" [N, outputs].
    rotary: overrides spec["rotary"] (the same tables, another spelling)."""
    rot = rotary_options(rotary) if rotary is not None else spec.get("rotary")
    T, E, hq, hkv = spec["T"], spec["E"], spec["hq"], spec["hkv"]
    nodes, inits = [], []
    f32 = lambda name, v: inits.append(tensor(name, np.asarray(v, dtype=np.float32)))  # noqa: E731

    def matmul(x, W, out, name):
        f32(name + "_W", W)
        nodes.append(node("MatMul", [x, name + "_W"], [out], name=name))
        return out

    def rms(x, g, out, name):
        f32(name + "_g", g)
        nodes.append(node("RMSNormalization", [x, name + "_g"], [out], [attr_i("axis", -1), attr_f("epsilon", spec["eps"])], name=name))
        return out

    inits.append(tensor("flat_shape", np.asarray([-1, T, E], dtype=np.int64)))
    nodes.append(node("Reshape", ["X", "flat_shape"], ["X3"]))
    x = "X3"
    for i, L in enumerate(spec["layers"]):
        p = f"l{i}_"
        a_in = rms(x, L["g1"], p + "n1", p + "norm1")
        q, k, v = (matmul(a_in, L["W" + c], p + c, p + c + "_proj") for c in "qkv")
        a = attention_op_nodes(nodes, inits, p + "a_", q, k, v, T, T, hq, hkv, E // hq, form=form, causal=True, **({} if rot is None else {"rotary": rot}))
        a = matmul(a, L["Wo"], p + "ao", p + "out_proj")
        nodes.append(node("Add", [x, a], [p + "r1"], name=p + "res1"))
        x = p + "r1"
        f_in = rms(x, L["g2"], p + "n2", p + "norm2")
        gate, up = matmul(f_in, L["Wg"], p + "gate", p + "gate_proj"), matmul(f_in, L["Wu"], p + "up", p + "up_proj")
        nodes += [node("Sigmoid", [gate], [p + "sg"], name=p + "sigmoid"), node("Mul", [gate, p + "sg"], [p + "sw"], name=p + "swish"),
                  node("Mul", [p + "sw", up], [p + "glu"], name=p + "glu_mul")]
        f = matmul(p + "glu", L["Wd"], p + "down", p + "down_proj")
        nodes.append(node("Add", [x, f], [p + "r2"], name=p + "res2"))
        x = p + "r2"
    x = rms(x, spec["g_final"], "dec", "final_norm")
    inits.append(tensor("last_i", np.asarray(-1, dtype=np.int64)))
    nodes.append(node("Gather", [x, "last_i"], ["last_t"], [attr_i("axis", 1)], name="last_step"))
    f32("head_b", spec["head_b"])
    matmul("last_t", spec["head_W"], "last_mm", "last_head")
    nodes.append(node("Add", ["last_mm", "head_b"], ["last"], name="last_head_bias"))
    return model("decoder", nodes, inits, [value_info("X", ["N", T * E])], [value_info("last", ["N", int(np.asarray(spec["head_W"]).shape[1])])], opset=opset)


def decoder_block_reference(spec: dict, x, rotary=None) -> np.ndarray:
    """float64 numpy restatement of decoder_block_from_spec(spec): x [N, T E] -> [N, outputs]."""
    T, E, hq, hkv = spec["T"], spec["E"], spec["hq"], spec["hkv"]
    rot = rotary_options(rotary) if rotary is not None else spec.get("rotary")
    rope = (lambda a, h: a) if rot is None else (lambda a, h: rotary_apply(a, T, h, E // hq, rot, np.float64))  # noqa: E731
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    x = f64(x).reshape(-1, T, E)
    for L in spec["layers"]:
        a_in = rmsnorm_reference(x, L["g1"], spec["eps"])
        a = attention_op_reference(rope(a_in @ f64(L["Wq"]), hq), rope(a_in @ f64(L["Wk"]), hkv), a_in @ f64(L["Wv"]), hq, hkv, causal=True)
        x = x + a @ f64(L["Wo"])
        f_in = rmsnorm_reference(x, L["g2"], spec["eps"])
        gate = f_in @ f64(L["Wg"])
        x = x + (gate / (1.0 + np.exp(-gate)) * (f_in @ f64(L["Wu"]))) @ f64(L["Wd"])
    x = rmsnorm_reference(x, spec["g_final"], spec["eps"])
    return x[:, -1] @ f64(spec["head_W"]) + f64(spec["head_b"])


# ------------------------------------------------------------------------------------------
# Rotary position embeddings: the opset-23 operator RotaryEmbedding and the rotate_half spelling
# ------------------------------------------------------------------------------------------

def rotary_tables(T: int, rd: int, base: float = 10000.0, positions=None) -> tuple[np.ndarray, np.ndarray]:
    """(cos, sin), each [T, rd / 2] float32 (or one row per entry of positions): the angle p * base ** (-2 i / rd) of position p and pair i in
    float64, its cosine and sine in float64, rounded once to float32."""
    assert rd >= 2 and rd % 2 == 0
    pos = np.arange(T, dtype=np.float64) if positions is None else np.asarray(positions, dtype=np.float64)
    ang = pos[:, None] * np.float64(base) ** (-2.0 * np.arange(rd // 2, dtype=np.float64) / rd)[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def rotary_options(rotary) -> dict | None:
    """The rotary= keyword of the attention and decoder writers, normalised: None / False: off; True: the defaults; a dict: over the defaults.
    form: "op" (RotaryEmbedding), "slice" or "split" (the rotate_half spelling with two Slices / one Split); interleaved, rd (0 = dh), base;
    positions: None (0 .. T - 1) or a list of T constant positions into caches of cache_rows rows (the operator's position_ids);
    on: which operands are rotated, "qk"; slice_end: "exact" or "max" (INT64_MAX as the second Slice's end); table_rank: 2, 3 or 4 (the
    spelling's tables as [T, dh], [1, T, dh] or [1, 1, T, dh]); swap: the spelling's Add and Mul operands in the other order; break_:
    rotate_half_nodes."""
    if rotary is None or rotary is False:
        return None
    o = {"form": "op", "interleaved": False, "rd": 0, "base": 10000.0, "positions": None, "cache_rows": None, "on": "qk", "slice_end": "exact",
         "table_rank": 2, "swap": False, "break_": None}
    if isinstance(rotary, dict):
        assert not set(rotary) - set(o), set(rotary) - set(o)
        o.update(rotary)
    return o


def rotary_factors(cos, sin, interleaved: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """The step's factor tables A, B [T, rd] of cos, sin [T, rd / 2]: A = cos over both members of a pair, B = -sin on the first member and
    +sin on the second (pairs (j, j + rd / 2), or (2 i, 2 i + 1) when interleaved)."""
    cos, sin = np.asarray(cos), np.asarray(sin)
    if interleaved:
        return np.repeat(cos, 2, axis=1), np.stack([-sin, sin], axis=2).reshape(len(sin), -1)
    return np.concatenate([cos, cos], axis=1), np.concatenate([-sin, sin], axis=1)


def rotary_reference(x, A, B, h: int, dh: int, interleaved: bool = False, dtype=np.float32) -> np.ndarray:
    """The Rotary step's definition over x [N, T, h dh] with factor tables A, B [T, rd]: for column j < rd of every head
    out[j] = fl(fl(x[j] A[t, j]) + fl(x[partner(j)] B[t, j])), partner(j) = j +- rd / 2 or j ^ 1 (interleaved); columns j >= rd are copies.
    dtype float32: three separately rounded operations (the step's bits); float64: the same formula on the same float32 tables."""
    x = np.asarray(x, dtype=dtype)
    N, T = x.shape[:2]
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    rd = A.shape[1]
    x4 = x.reshape(N, T, h, dh)
    j = np.arange(rd)
    partner = (j ^ 1) if interleaved else np.where(j < rd // 2, j + rd // 2, j - rd // 2)
    out = x4.copy()
    with np.errstate(all="ignore"):
        out[..., :rd] = x4[..., :rd] * A[None, :, None, :] + x4[..., partner] * B[None, :, None, :]
    return out.reshape(N, T, h * dh)


def _rotary_caches(T: int, dh: int, rot: dict):
    """(cos, sin, positions or None) of the options: the caches as the operator reads them ([T, rd/2], or [cache_rows, rd/2] beside positions)."""
    rd = rot["rd"] or dh
    if rot["positions"] is None:
        return rotary_tables(T, rd, rot["base"]) + (None,)
    pos = [int(p) for p in rot["positions"]]
    assert len(pos) == T
    return rotary_tables(rot["cache_rows"] or max(pos) + 1, rd, rot["base"]) + (pos,)


def rotary_apply(x, T: int, h: int, dh: int, rotary, dtype=np.float32) -> np.ndarray:
    """rotary_reference over x [N, T, h dh] (or [N, T h dh]) with the tables of the options."""
    rot = rotary_options(rotary)
    cos, sin, pos = _rotary_caches(T, dh, rot)
    if pos is not None:
        cos, sin = cos[pos], sin[pos]
    A, B = rotary_factors(cos, sin, rot["interleaved"])
    return rotary_reference(np.asarray(x).reshape(-1, T, h * dh), A, B, h, dh, rot["interleaved"], dtype)


def rotary_op_nodes(nodes: list, inits: list, p: str, x: str, cos, sin, interleaved: bool = False, rd: int = 0, num_heads: int = 0, positions=None,
                    extra_attrs: Sequence[bytes] = (), domain: str = "") -> str:
    """Appends one RotaryEmbedding node '<p>rope' over x ([N, h, T, dh], or [N, T, h dh] beside num_heads) and returns its result.  cos, sin:
    [T, rd/2] arrays, stored as [1, T, rd/2]; beside positions (a list, stored as position_ids int64 [1, T]) as they are, [P, rd/2]."""
    cos, sin = np.asarray(cos, dtype=np.float32), np.asarray(sin, dtype=np.float32)
    if positions is None:
        cos, sin = cos[None], sin[None]
    inits += [tensor(p + "cos", cos), tensor(p + "sin", sin)]
    ins = [x, p + "cos", p + "sin"]
    if positions is not None:
        inits.append(tensor(p + "pos", np.asarray(positions, dtype=np.int64).reshape(1, -1)))
        ins.append(p + "pos")
    attrs = ([attr_i("interleaved", 1)] if interleaved else []) + ([attr_i("num_heads", num_heads)] if num_heads else []) + \
            ([attr_i("rotary_embedding_dim", rd)] if rd else [])
    nodes.append(node("RotaryEmbedding", ins, [p + "rot"], attrs + list(extra_attrs), name=p + "rope", domain=domain))
    return p + "rot"


def rotate_half_nodes(nodes: list, inits: list, p: str, x: str, cos_full, sin_full, halves: str = "slice", slice_end: str = "exact", table_rank: int = 2,
                      swap: bool = False, break_: str | None = None) -> str:
    """Appends Hugging Face's apply_rotary_pos_emb over x [N, h, T, dh], x * cos + rotate_half(x) * sin with rotate_half(x) = cat(-x2, x1), and
    returns its result (node '<p>add').  cos_full, sin_full: [T, dh]; halves: two Slices of the last axis or one Split; swap: Add and Mul
    operands in the other order.  break_: a sub-graph that is NOT the embedding -- "bounds" (the second Slice starts one column late) or
    "order" (cat(x1, -x2))."""
    cos_full, sin_full = np.asarray(cos_full, dtype=np.float32), np.asarray(sin_full, dtype=np.float32)
    d = cos_full.shape[-1]
    lead = (1,) * (table_rank - 2)
    inits += [tensor(p + "cos", cos_full.reshape(lead + cos_full.shape)), tensor(p + "sin", sin_full.reshape(lead + sin_full.shape))]
    i64 = lambda name, val: inits.append(tensor(name, np.asarray(val, dtype=np.int64)))  # noqa: E731
    if halves == "split":
        i64(p + "sp", [d // 2, d // 2])
        nodes.append(node("Split", [x, p + "sp"], [p + "x1", p + "x2"], [attr_i("axis", -1)], name=p + "split"))
    else:
        i64(p + "b0", [0]); i64(p + "b1", [d // 2 + (1 if break_ == "bounds" else 0)]); i64(p + "e1", [d // 2])  # noqa: E702
        i64(p + "e2", [np.iinfo(np.int64).max if slice_end == "max" else d]); i64(p + "ax", [-1])  # noqa: E702
        nodes += [node("Slice", [x, p + "b0", p + "e1", p + "ax"], [p + "x1"], name=p + "slice1"),
                  node("Slice", [x, p + "b1", p + "e2", p + "ax"], [p + "x2"], name=p + "slice2")]
    if break_ == "order":
        nodes += [node("Neg", [p + "x2"], [p + "nx2"], name=p + "neg"), node("Concat", [p + "x1", p + "nx2"], [p + "rh"], [attr_i("axis", -1)], name=p + "cat")]
    else:
        nodes += [node("Neg", [p + "x2"], [p + "nx2"], name=p + "neg"), node("Concat", [p + "nx2", p + "x1"], [p + "rh"], [attr_i("axis", -1)], name=p + "cat")]
    pair = lambda a, b: [b, a] if swap else [a, b]  # noqa: E731
    nodes += [node("Mul", pair(x, p + "cos"), [p + "xc"], name=p + "mul_cos"), node("Mul", pair(p + "rh", p + "sin"), [p + "rs"], name=p + "mul_sin"),
              node("Add", pair(p + "xc", p + "rs"), [p + "rot"], name=p + "add")]
    return p + "rot"


def rotary_nodes(nodes: list, inits: list, p: str, x: str, T: int, dh: int, rotary, num_heads: int = 0) -> str:
    """The rotary embedding of the options (rotary_options) over x: head-major [N, h, T, dh], or [N, T, h dh] beside num_heads (form "op" only)."""
    rot = rotary_options(rotary)
    cos, sin, pos = _rotary_caches(T, dh, rot)
    if rot["form"] == "op":
        return rotary_op_nodes(nodes, inits, p, x, cos, sin, rot["interleaved"], rot["rd"], num_heads, pos)
    assert not num_heads and not rot["interleaved"] and (rot["rd"] or dh) == dh, "the rotate_half spelling: head-major, half pairing, whole heads"
    if pos is not None:
        cos, sin = cos[pos], sin[pos]
    return rotate_half_nodes(nodes, inits, p, x, np.concatenate([cos, cos], axis=1), np.concatenate([sin, sin], axis=1), rot["form"], rot["slice_end"],
                             rot["table_rank"], rot["swap"], rot["break_"])


def rotary_model(T: int, h: int, dh: int, rotary=True, opset: int = 23, batch: int | str = "N", **kw) -> bytes:
    """The 3-D operator alone: X [N, T h dh] -> Reshape [N, T, h dh] -> RotaryEmbedding(num_heads = h) -> output [N, T, h dh]; node 'r_rope'.
    kw: rotary_op_nodes (extra_attrs, domain, num_heads = another count or 0)."""
    rot = rotary_options(rotary)
    assert rot["form"] == "op"
    E = h * dh
    cos, sin, pos = _rotary_caches(T, dh, rot)
    nodes, inits = [node("Reshape", ["X", "x_shape"], ["x3"])], [tensor("x_shape", np.asarray([-1, T, E], dtype=np.int64))]
    out = rotary_op_nodes(nodes, inits, "r_", "x3", cos, sin, rot["interleaved"], rot["rd"], kw.pop("num_heads", h), pos, **kw)
    return model("rotary", nodes, inits, [value_info("X", [batch, T * E])], [value_info(out, [batch, T, E])], opset=opset)


# ------------------------------------------------------------------------------------------
# Sub-pixel layers: DepthToSpace, SpaceToDepth and their Reshape -> Transpose -> Reshape spellings
# ------------------------------------------------------------------------------------------
# form -> (the first Reshape's 6-D target, by name; the Transpose's perm).  b1 / b2 = the block's rows / columns, Cs = C / (b1 b2)
PIXEL_SHUFFLE_SPELLINGS = {
    "dcr": (("N", "b1", "b2", "Cs", "H", "W"), (0, 3, 4, 1, 5, 2)),
    "crd": (("N", "Cs", "b1", "b2", "H", "W"), (0, 1, 4, 2, 5, 3)),
    "s2d": (("N", "C", "Hb", "b1", "Wb", "b2"), (0, 3, 5, 1, 2, 4)),
    "unshuffle": (("N", "C", "Hb", "b1", "Wb", "b2"), (0, 1, 3, 5, 2, 4)),
}


def pixel_shuffle_apply(x, form: str, b) -> np.ndarray:
    """A sub-pixel layer over x [N, C, H, W] as the specification writes it: reshape to six axes, transpose, reshape.  The values are moved,
    never changed, so the result has x's dtype.  b: the block size or (b_h, b_w)."""
    x = np.asarray(x)
    bh, bw = _pair(b)
    n, c, h, w = x.shape
    six, perm = PIXEL_SHUFFLE_SPELLINGS[form]
    dims = dict(N=n, b1=bh, b2=bw, Cs=c // (bh * bw), C=c, H=h, W=w, Hb=h // bh, Wb=w // bw)
    out = (n, c // (bh * bw), h * bh, w * bw) if form in ("dcr", "crd") else (n, c * bh * bw, h // bh, w // bw)
    return x.reshape([dims[k] for k in six]).transpose(perm).reshape(out)


def pixel_shuffle_model(form: str = "crd", b=2, c: int = 16, hw=(3, 5), spelling: bool = False, pre: bool = False, post: bool = False, opset: int = 13,
                        extra_outputs: Sequence[str] = (), **kw) -> tuple[bytes, dict]:
    """One sub-pixel layer 'ps' over X [N, c, *hw] (_DecoderNet.shuffle has the forms and the spelling's options).  pre: an identity 1x1 Conv in
    front (the layer then reads a channel-quad tensor where c is whole quads); post: an identity 1x1 ConvTranspose behind it (the layer then
    writes one).  extra_outputs: further graph outputs by value name ('ps_6d', 'ps_t': the spelling's intermediates).  Returns (model, spec)."""
    net = _DecoderNet(0)
    cur = "X"
    if pre:
        cur = net.conv(cur, c, c, 1, 1, 0, bias=False, w=np.eye(c, dtype=np.float32)[:, :, None, None])
    cur, oshape = net.shuffle(cur, c, hw, form, b, spelling=spelling, name="ps", **kw)
    if post:
        cur = net.convt(cur, oshape[0], oshape[0], 1, 1, 0, bias=False, w=np.eye(oshape[0], dtype=np.float32)[:, :, None, None])
    in_shape = (c,) + tuple(hw)
    spec = {"layers": net.layers, "output": cur, "in_shape": in_shape, "out_shape": oshape}
    outs = [value_info(cur, ["N"] + list(oshape))] + [value_info(o, []) for o in extra_outputs]
    return model("pixel_shuffle", net.nodes, net.inits, [value_info("X", ["N"] + list(in_shape))], outs, opset=opset), spec


def pixel_shuffle_pair_model(form: str = "crd", b: int = 2, c: int = 16, hw=(3, 5), pre: bool = False, post: bool = False) -> tuple[bytes, dict]:
    """DepthToSpace of X [N, c, *hw] followed by the matching space-to-depth form (dcr: SpaceToDepth; crd: the pixel_unshuffle spelling): the
    identity.  pre / post as in pixel_shuffle_model."""
    net = _DecoderNet(0)
    cur = "X"
    if pre:
        cur = net.conv(cur, c, c, 1, 1, 0, bias=False, w=np.eye(c, dtype=np.float32)[:, :, None, None])
    cur, mid = net.shuffle(cur, c, hw, form, b, name="up")
    cur, back = net.shuffle(cur, mid[0], mid[1:], "s2d" if form == "dcr" else "unshuffle", b, spelling=form != "dcr", name="down")
    if post:
        cur = net.convt(cur, c, c, 1, 1, 0, bias=False, w=np.eye(c, dtype=np.float32)[:, :, None, None])
    in_shape = (c,) + tuple(hw)
    return net.finish("pixel_shuffle_pair", value_info("X", ["N"] + list(in_shape)), cur, ["N"] + list(in_shape), extra={"in_shape": in_shape, "out_shape": tuple(back)})


def espcn(b: int = 2, in_ch: int = 3, size: int = 12, widths: Sequence[int] = (16, 8), seed: int = 91, spelling: bool = False, opset: int = 13) -> tuple[bytes, dict]:
    """ESPCN-shaped super-resolution: Conv 5x5 + Tanh -> Conv 3x3 + Tanh -> Conv 3x3 to in_ch * b^2 channels -> PixelShuffle (DepthToSpace CRD, what
    torch writes for nn.PixelShuffle from opset 11 on; spelling: the Reshape -> Transpose -> Reshape form of older opsets)."""
    net = _DecoderNet(seed)
    cur = net.act(net.conv("X", in_ch, widths[0], 5, 1, 2), "Tanh")
    cur = net.act(net.conv(cur, widths[0], widths[1], 3, 1, 1), "Tanh")
    cur = net.conv(cur, widths[1], in_ch * b * b, 3, 1, 1)
    cur, oshape = net.shuffle(cur, in_ch * b * b, (size, size), "crd", b, spelling=spelling, name="ps")
    return net.finish("espcn", value_info("X", ["N", in_ch, size, size]), cur, ["N"] + list(oshape), opset=opset, extra={"in_shape": (in_ch, size, size), "out_shape": oshape})


def pixel_unshuffle_stem(b: int = 2, in_ch: int = 3, size: int = 12, width: int = 16, classes: int = 8, seed: int = 93) -> tuple[bytes, dict]:
    """The SpaceToDepth stem of TResNet / Real-ESRGAN: pixel_unshuffle of the image (its Reshape -> Transpose -> Reshape spelling) -> Conv 3x3 + Relu
    -> Conv 1x1 to `classes` channels -> GlobalAveragePool -> Flatten: [N, classes]."""
    net = _DecoderNet(seed)
    cur, s = net.shuffle("X", in_ch, (size, size), "unshuffle", b, spelling=True, name="ps")
    cur = net.act(net.conv(cur, s[0], width, 3, 1, 1), "Relu")
    cur = net.conv(cur, width, classes, 1, 1, 0)
    net.nodes.append(node("GlobalAveragePool", [cur], ["gap"], name="gap"))
    net.layers.append(("gap", "gap", [cur], {}))
    net.nodes.append(node("Flatten", ["gap"], ["scores"], [attr_i("axis", 1)], name="flatten"))
    net.layers.append(("reshape", "scores", ["gap"], dict(shape=(classes,))))
    return net.finish("pixel_unshuffle_stem", value_info("X", ["N", in_ch, size, size]), "scores", ["N", classes], extra={"in_shape": (in_ch, size, size)})
