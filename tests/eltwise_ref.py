"""A float64 restatement of the elementwise operators (hip/eltwise.hip, apply_act_c in hip/device_common.hpp and its uses in the MFMA
epilogues) and of the row kernels (Softmax, LogSoftmax, Normalizer), from numpy alone, over the whole float32 range.  A helper module
(tests/test_eltwise_ref.py checks it and the CPU oracle without a GPU, tests/test_eltwise_range_gpu.py uses it on one), not a conftest.

Every reference is the ONNX definition evaluated in float64 from the float32 input, written so that float64 itself does not overflow
(Softplus as logaddexp(0, v), Sigmoid and Swish by the sign of v, Elu and Selu through expm1).  Attribute constants go through float32
first: the kernels hold them as f32.

verdict(): ONE rule.  Where the reference rounded to float32 is NaN the result is NaN, where it is +-inf the result is that infinity,
elsewhere the result is finite and within the project bar 1e-4 |ref| + 1e-6.  Floor, Ceil and Round are equal outright: every SWEEP value
is a float32, so their result has one right answer (ties to even included).

NaN.  Arithmetic-defined operators propagate NaN and the float64 reference says so.  The comparison-defined ones (Relu, LeakyRelu, Clip,
HardSigmoid, HardSwish; Min / Max / PRelu against a constant) are defined by the C expression in oracle/infera_oracle.c, whose value at
NaN is NAN_TABLE below -- a comparison with NaN is false, fminf / fmaxf return their other operand."""
from __future__ import annotations

import math

import numpy as np

from infera_amd import onnx_writer as W

RTOL, ATOL = 1e-4, 1e-6
f32 = np.float32

_POS = [1e-45, 1e-38, 1e-20, 1e-7, 1e-3, 0.5, 1.0, 1.5, 2.5, 3.0, 5.0, 6.0, 8.0, 10.0, 17.0, 20.0, 50.0, 87.0, 88.5, 89.0, 100.0, 104.0, 1e4, 1e30, 3e38]
SWEEP = np.array([0.0, -0.0] + [s * v for v in _POS for s in (1.0, -1.0)] + [1e-40, 0.999999, 1.0000001, 3.5, np.inf, -np.inf, np.nan], dtype=np.float32)
FINITE = SWEEP[np.isfinite(SWEEP)]

_erf = np.vectorize(math.erf, otypes=[np.float64])


def _c(v):
    """an attribute as the kernels hold it"""
    return np.float64(np.float32(v))


def _sigmoid(v):
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(v))  # never above 1
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))  # (a NaN v makes e NaN: both branches are)


def _hard_sigmoid(v, a, b):
    return np.clip(_c(a) * v + _c(b), 0.0, 1.0)


SELU_ALPHA, SELU_GAMMA = 1.67326319217681884765625, 1.05070102214813232421875

# name -> (ONNX operator, {attribute: value}, float64 definition).  Clip's bounds are inputs (opset 13).
UNARY = {
    "Relu": ("Relu", {}, lambda v: np.maximum(v, 0.0)),
    "Sigmoid": ("Sigmoid", {}, _sigmoid),
    "Tanh": ("Tanh", {}, np.tanh),
    "LeakyRelu": ("LeakyRelu", {"alpha": 0.1}, lambda v: np.where(v >= 0, v, _c(0.1) * v)),
    "Clip": ("Clip", {"min": -2.5, "max": 6.0}, lambda v: np.clip(v, -2.5, 6.0)),
    "Clip-open": ("Clip", {"min": -1.0}, lambda v: np.maximum(v, -1.0)),
    "Exp": ("Exp", {}, np.exp),
    "Log": ("Log", {}, np.log),
    "Sqrt": ("Sqrt", {}, np.sqrt),
    "Neg": ("Neg", {}, np.negative),
    "Abs": ("Abs", {}, np.abs),
    "Elu": ("Elu", {}, lambda v: np.where(v >= 0, v, np.expm1(np.minimum(v, 0.0)))),
    "Elu-0.7": ("Elu", {"alpha": 0.7}, lambda v: np.where(v >= 0, v, _c(0.7) * np.expm1(np.minimum(v, 0.0)))),
    "Selu": ("Selu", {}, lambda v: _c(SELU_GAMMA) * np.where(v > 0, v, _c(SELU_ALPHA) * np.expm1(np.minimum(v, 0.0)))),
    "Selu-1.2-0.9": ("Selu", {"alpha": 1.2, "gamma": 0.9}, lambda v: _c(0.9) * np.where(v > 0, v, _c(1.2) * np.expm1(np.minimum(v, 0.0)))),
    "Softplus": ("Softplus", {}, lambda v: np.logaddexp(0.0, v)),
    "HardSigmoid": ("HardSigmoid", {}, lambda v: _hard_sigmoid(v, 0.2, 0.5)),
    "HardSigmoid-0.3-0.4": ("HardSigmoid", {"alpha": 0.3, "beta": 0.4}, lambda v: _hard_sigmoid(v, 0.3, 0.4)),
    "HardSwish": ("HardSwish", {}, lambda v: v * np.clip(v / 6.0 + 0.5, 0.0, 1.0)),
    "Erf": ("Erf", {}, _erf),
    "Gelu": ("Gelu", {}, lambda v: 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))),
    "Reciprocal": ("Reciprocal", {}, lambda v: 1.0 / v),
    "Floor": ("Floor", {}, np.floor),
    "Ceil": ("Ceil", {}, np.ceil),
    "Softsign": ("Softsign", {}, lambda v: v / (1.0 + np.abs(v))),
    "Round": ("Round", {}, np.rint),
    "Swish": ("Swish", {}, lambda v: v * _sigmoid(v)),  # spelled x * Sigmoid(x)
}
OPERATORS = sorted({op for op, _, _ in UNARY.values()} - {"Swish"})  # lowering.cpp's unary set: 22 names
EXACT = ("Floor", "Ceil", "Round")
MFMA_FUSABLE = ("Relu", "Sigmoid", "Tanh", "LeakyRelu", "Clip", "HardSigmoid", "HardSwish", "Swish")  # lowering: mfma_fusable
KINDS_1_TO_5 = MFMA_FUSABLE[:5]  # what the ConvTranspose2d and HDense epilogues take

# The value at NaN of each comparison-defined operator: its C expression in oracle/infera_oracle.c, evaluated at v = NaN.
#   Relu         v > 0 ? v : 0                                  -> 0
#   LeakyRelu    v >= 0 ? v : alpha v                           -> NaN
#   Clip         v < lo ? lo : (v > hi ? hi : v)                -> NaN
#   HardSigmoid  fmaxf(0, fminf(1, alpha v + beta))             -> 1
#   HardSwish    v fmaxf(0, fminf(1, v / 6 + 0.5))              -> NaN
#   Min, Max     fminf(v, c), fmaxf(v, c)                       -> c
#   PRelu        v >= 0 ? v : c v                               -> NaN
# None stands for "the constant operand".
NAN_TABLE = {"Relu": 0.0, "LeakyRelu": np.nan, "Clip": np.nan, "HardSigmoid": 1.0, "HardSwish": np.nan, "Min": None, "Max": None, "PRelu": np.nan}


def reference(name, x):
    """the float64 definition of UNARY[name] at the float32 values x, NAN_TABLE applied"""
    op, _, fn = UNARY[name]
    x = np.asarray(x)
    assert x.dtype == np.float32
    with np.errstate(all="ignore"):
        ref = np.asarray(fn(x.astype(np.float64)), np.float64)
    if op in NAN_TABLE:
        ref = np.where(np.isnan(x), NAN_TABLE[op], ref)
    return ref


def verdict_ref(got, ref, exact: bool = False):
    """(ok, ratio) per element of a float32 result against a float64 reference: the module docstring's rule; ratio = error / bar where
    both are finite, 0 where a NaN or an infinity is matched, inf where the rule is broken"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(ref), (got.dtype, got.shape, np.shape(ref))
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        r32 = ref.astype(np.float32)
        g64 = got.astype(np.float64)
        nan, inf = np.isnan(r32), np.isinf(r32)
        ratio = np.abs(g64 - ref) / (RTOL * np.abs(ref) + ATOL)
    if exact:
        ok = np.where(nan, np.isnan(got), got == r32)
    else:
        ok = np.where(nan, np.isnan(got), np.where(inf, got == r32, np.isfinite(got) & (ratio <= 1.0)))
    ratio = np.where(nan | inf, 0.0, ratio)
    return ok, np.where(ok, ratio, np.inf)


def verdict(got, x, op):
    """(ok, ratio) per element of `got` = op(x); op is a key of UNARY"""
    return verdict_ref(got, reference(op, x), exact=UNARY[op][0] in EXACT)


def describe(ok, x, got, ref):
    """the first few misses, for an assertion message"""
    idx = np.argwhere(~ok)[:8]
    return [(tuple(i), float(np.asarray(x)[tuple(i)]), float(got[tuple(i)]), float(np.asarray(ref)[tuple(i)])) for i in idx]


def sweep_table(rows: int, cols: int = 7, values=SWEEP):
    """`values` tiled into [rows, cols], each row count starting at another element"""
    return np.resize(np.roll(values, -3 * rows), rows * cols).reshape(rows, cols).astype(np.float32)


# ---- graphs -----------------------------------------------------------------------------------------------------------------------

def unary_nodes(name, src, dst, inits, tag=""):
    """the nodes of UNARY[name] reading `src` and writing `dst`; constants go to `inits`"""
    op, attrs, _ = UNARY[name]
    if op == "Swish":
        return [W.node("Sigmoid", [src], [dst + "_sg"]), W.node("Mul", [src, dst + "_sg"], [dst])]
    if op == "Clip":
        ins = [src]
        for k in ("min", "max"):
            if k in attrs:
                inits.append(W.tensor(f"{dst}_{k}{tag}", np.array(attrs[k], np.float32)))
                ins.append(f"{dst}_{k}{tag}")
        return [W.node("Clip", ins, [dst])]
    return [W.node(op, [src], [dst], [W.attr_f(k, v) for k, v in attrs.items()])]


def unary_graph(name, cols: int) -> bytes:
    """Y = Op(X) on [N, cols]: an activation of the graph input has no producer to fuse into"""
    inits = []
    nodes = unary_nodes(name, "X", "Y", inits)
    return W.model("eltwise_" + name, nodes, inits, [W.value_info("X", ["N", cols])], [W.value_info("Y", ["N", cols])], opset=20 if name == "Gelu" else 13)


def act_name(name):
    """what the plan calls the activation"""
    return UNARY[name][0]


def select01(K: int, M: int):
    """a 0/1 selection K -> M (column m copies input (a m + c) mod K, a coprime to K, the last column the last input) and the sources"""
    a = next(s for s in (7, 5, 3, 2, 1) if math.gcd(s, K) == 1)
    src = (a * np.arange(M) + (K - 1 - a * (M - 1))) % K
    w = np.zeros((K, M), np.float32)
    w[src, np.arange(M)] = 1.0
    return w, src


# ---- binaries ---------------------------------------------------------------------------------------------------------------------

BINARY = ("Add", "Sub", "Mul", "Div", "Min", "Max", "Pow", "PRelu")


def binary64(op, a, b):
    """a (op) b in float64 from float32 operands; PRelu: b is the slope; Min / Max as fminf / fmaxf"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        if op == "Add":
            return a + b
        if op == "Sub":
            return a - b
        if op == "Mul":
            return a * b
        if op == "Div":
            return a / b
        if op == "Min":
            return np.fmin(a, b)
        if op == "Max":
            return np.fmax(a, b)
        if op == "Pow":
            return np.power(a, b)
        assert op == "PRelu", op
        return np.where(a >= 0, a, b * a)


# ---- rows -------------------------------------------------------------------------------------------------------------------------

REGIMES = ("a", "b+", "b-", "c", "d0", "d88", "d-1e30", "e", "f", "g", "h-nan", "h+inf", "h-inf")
HEAD_REGIMES = tuple(r for r in REGIMES if r[0] not in "fh")  # what the fused heads are asked: finite logits


def softmax_rows(length: int, seed: int = 0, rows: int = 67, regimes=REGIMES):
    """(x [rows, length] f32, the regime of each row): the rows cycle through `regimes`, so the vectors that share a wave differ.
    a: uniform +-4; b+-: the same row +-1e4; c: uniform +-60; d*: all elements equal; e: one element 100 above the rest;
    f: -inf at a third of the positions (j % 3 == 1; at least one position stays); g: 3e38 and -3e38 alternating;
    h*: a single NaN, a single +inf, all -inf"""
    rng = np.random.default_rng([seed, length])
    x = np.empty((rows, length), np.float32)
    names = [regimes[r % len(regimes)] for r in range(rows)]
    for r, name in enumerate(names):
        u = rng.uniform(-4.0, 4.0, length).astype(np.float32)
        if name == "b+":
            u = u + f32(1e4)
        elif name == "b-":
            u = u - f32(1e4)
        elif name == "c":
            u = (u * f32(15.0)).astype(np.float32)
        elif name[0] == "d":
            u[:] = {"d0": 0.0, "d88": 88.0, "d-1e30": -1e30}[name]
        elif name == "e":
            u[r % length] = u.max() + f32(100.0)
        elif name == "f":
            u[1::3] = -np.inf
        elif name == "g":
            u[0::2], u[1::2] = 3e38, -3e38
        elif name == "h-nan":
            u[(3 * r) % length] = np.nan
        elif name == "h+inf":
            u[(3 * r) % length] = np.inf
        elif name == "h-inf":
            u[:] = -np.inf
        x[r] = u
    return x, names


def softmax64(x, log: bool = False):
    """Softmax / LogSoftmax over the last axis in float64, the maximum subtracted"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        s = x - np.max(x, axis=-1, keepdims=True)  # (np.max propagates NaN: the row is NaN)
        e = np.exp(s)
        total = e.sum(-1, keepdims=True)
        return s - np.log(total) if log else e / total


NORM_FLOOR = np.float64(np.float32(1e-30))
NORMS = ("L1", "L2", "MAX")
NORM_REGIMES = ("a", "a*1e15", "a*1e-15", "zero", "nan")


def normalizer_rows(length: int, seed: int = 0, rows: int = 67):
    """(x, the regime of each row): uniform +-4; that times 1e15 and 1e-15 (the f32 sum of squares stays a normal number); a zero row;
    a row with one NaN"""
    rng = np.random.default_rng([seed, length, 7])
    x = np.empty((rows, length), np.float32)
    names = [NORM_REGIMES[r % len(NORM_REGIMES)] for r in range(rows)]
    for r, name in enumerate(names):
        u = rng.uniform(-4.0, 4.0, length).astype(np.float32)
        if name == "a*1e15":
            u = u * f32(1e15)
        elif name == "a*1e-15":
            u = u * f32(1e-15)
        elif name == "zero":
            u[:] = 0.0
        elif name == "nan":
            u[(3 * r) % length] = np.nan
        x[r] = u
    return x, names


def normalizer64(x, norm: str):
    """x / max(norm(x), 1e-30) per row: L1 = sum |x|, L2 = sqrt(sum x^2), MAX = max |x| by comparisons (fmaxf: a NaN element is passed
    over, so only that element of a MAX row is NaN; a sum carries it to the whole row)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if norm == "L1":
            d = np.abs(x).sum(-1, keepdims=True)
        elif norm == "L2":
            d = np.sqrt(np.square(x).sum(-1, keepdims=True))
        else:
            assert norm == "MAX", norm
            d = np.fmax.reduce(np.abs(x), axis=-1, keepdims=True, initial=0.0)
        return x / np.maximum(d, NORM_FLOOR)


def row_graph(op: str, length: int) -> bytes:
    """Softmax / LogSoftmax (axis 1) or NormL1 / NormL2 / NormMAX on [N, length]"""
    io = ([W.value_info("X", ["N", length])], [W.value_info("Y", ["N", length])])
    if op.startswith("Norm"):
        return W.model("rows", [W.node("Normalizer", ["X"], ["Y"], [W.attr_s("norm", op[4:])], domain=W.ML_DOMAIN)], [], *io, ml_opset=1)
    return W.model("rows", [W.node(op, ["X"], ["Y"], [W.attr_i("axis", 1)])], [], *io)


def row_reference(op: str, x):
    return normalizer64(x, op[4:]) if op.startswith("Norm") else softmax64(x, log=op == "LogSoftmax")


def row_batch(op: str, length: int, seed: int = 0, rows: int = 67):
    return normalizer_rows(length, seed, rows) if op.startswith("Norm") else softmax_rows(length, seed, rows)


def poisoned(names):
    """the rows of a batch that hold a NaN or an infinity where it spreads over the row"""
    return np.array([n[0] == "h" or n == "nan" for n in names])


def check_rows(op: str, x, names, got, clean):
    """the exact expectations and the float64 bar on one batch; `clean` is the same call with the poisoned rows replaced by zeros.
    Returns the worst ratio to the bar."""
    length = x.shape[1]
    ref = row_reference(op, x)
    ok, ratio = verdict_ref(got, ref)
    assert ok.all(), (op, length, [(names[i[0]],) + t for i, t in zip(np.argwhere(~ok)[:8], describe(ok, x, got, ref))])
    names = np.array(names)
    bad = poisoned(names)
    assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32)), (op, length, "a poisoned row changed its neighbours")
    if op in ("Softmax", "LogSoftmax"):
        assert np.isnan(got[bad]).all(), (op, length)
        eq = np.array([n[0] == "d" for n in names])
        if op == "Softmax":
            assert (got[eq] == np.float32(1) / np.float32(length)).all(), (op, length, got[eq][:, :2])
        masked = np.isneginf(x) & (names == "f")[:, None]
        assert (got[masked] == (0.0 if op == "Softmax" else -np.inf)).all(), (op, length)
    elif op != "NormMAX":
        assert np.isnan(got[bad]).all(), (op, length)
    return float(ratio.max())


# ---- binary graphs ----------------------------------------------------------------------------------------------------------------

def binary_const_graph(ops, consts, cols: int, left: bool = False) -> bytes:
    """X [N, cols] through a run of nodes `ops`, each against its own [cols] (or [1]) constant, on the left or on the right"""
    ops, consts = ([ops], [consts]) if isinstance(ops, str) else (list(ops), list(consts))
    nodes, inits, cur = [], [], "X"
    for i, (op, c) in enumerate(zip(ops, consts)):
        inits.append(W.tensor(f"C{i}", np.ascontiguousarray(c, np.float32)))
        out = "Y" if i == len(ops) - 1 else f"T{i}"
        nodes.append(W.node(op, [f"C{i}", cur] if left else [cur, f"C{i}"], [out]))
        cur = out
    return W.model("eltwise_const", nodes, inits, [W.value_info("X", ["N", cols])], [W.value_info("Y", ["N", cols])])


def binary_tensor_graph(op: str, cols: int, b_cols: int | None = None, swap: bool = False) -> bytes:
    """A [N, cols] (op) B [N, b_cols]: two graph inputs, served from one table whose columns are A's, then B's"""
    b_cols = cols if b_cols is None else b_cols
    ins = ["B", "A"] if swap else ["A", "B"]
    return W.model("eltwise_tensor", [W.node(op, ins, ["Y"])], [], [W.value_info("A", ["N", cols]), W.value_info("B", ["N", b_cols])],
                   [W.value_info("Y", ["N", cols])])


POW_EXPONENTS = np.array([2.0, 3.0, 0.0, 0.5, -1.0, 1.0, -2.0], np.float32)  # integer exponents take negative bases; 0^0 = 1; x^0.5
